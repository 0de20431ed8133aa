"""Adaptive key frames (SPEC §6.7) on a clip of a size users run: 16 frames of 700 x 700, a 16 px / frame pan with one cut in the middle, five levels, motion on, run four
ways — every frame full, the grid -key 4, nct_seq_frame_auto at the defaults, independent pairs. Prints one JSON line per way and a summary: the decisions, probe_ms, the
host wall time of propagated and full frames (every call ends in a synchronise), the transform flicker along the motion inside each scene and every frame's PSNR against
the all-full run. Each way runs REPS times after a warm-up pass over every path; times are medians, with the spread beside them.
usage: python scripts/seq_key_report.py [out.json] [--size 700] [--frames 16] [--step 16] [--reps 3]"""
import json
import statistics
import sys
import time

sys.path.insert(0, "tests"); sys.path.insert(0, "neural-color-transfer_amd/python")
import numpy as np
import nct, synth, seq_ref, seq_mc_ref, seq_prop_ref
from caffemodel_io import synthetic_vgg19


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


S, NF, STEP, REPS = arg("--size", 700), arg("--frames", 16), arg("--step", 16), arg("--reps", 3)
out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else None
half = NF // 2
frames = seq_ref.pan_frames(half, S, S, step=STEP) + seq_ref.pan_frames(NF - half, S, S, step=STEP, seed=2000)
ref = synth.image(2001, S, S)
ws, bs = synthetic_vgg19(19)
KIND = "FPKC"


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return r, 1e3 * (time.perf_counter() - t0)


def run(c, way):
    """-> (outputs, per-frame ms, kinds, decisions)"""
    outs, ms, kinds, ds = [], [], [], []
    if way == "pairs":
        for f in frames:
            o, t = timed(lambda: c.process_pair(f, ref))
            outs.append(o); ms.append(t); kinds.append("F")
        return outs, ms, kinds, ds
    c.seq_begin(ref, frames[0].shape)
    c.seq_set_motion()
    try:
        for k, f in enumerate(frames):
            if way == "auto":
                (o, d), t = timed(lambda: c.seq_frame_auto(f))
                kinds.append(KIND[d["kind"]]); ds.append(d)
            elif way == "key4" and k % 4:
                o, t = timed(lambda: c.seq_frame_propagate(f)); kinds.append("P")
            else:
                o, t = timed(lambda: c.seq_frame(f)); kinds.append("K" if k else "F")
            outs.append(o); ms.append(t)
    finally:
        c.seq_end()
    return outs, ms, kinds, ds


def scene_flicker(outs):
    a = seq_mc_ref.warped_flicker(outs[:half], frames[:half], STEP)[1]
    b = seq_mc_ref.warped_flicker(outs[half:], frames[half:], STEP)[1]
    return (a * (half - 1) + b * (NF - half - 1)) / (NF - 2)


def med(v):
    return None if not v else round(statistics.median(v), 3)


report = {"size": S, "frames": NF, "step": STEP, "reps": REPS, "ways": {}}
with nct.Context(0) as c:
    report["device"] = c.device_name()
    c.vgg19_load_raw(ws, bs)
    for way in ("full", "key4", "auto", "pairs"):              # warm-up: every path once, at the size that is timed
        saved, frames = frames, frames[:5]
        run(c, way)
        frames = saved
    full_outs = None
    for way in ("full", "key4", "auto", "pairs"):
        reps = [run(c, way) for _ in range(REPS)]
        outs, _, kinds, ds = reps[0]
        assert all(all(np.array_equal(a, b) for a, b in zip(outs, r[0])) for r in reps[1:]), "a repeat gave other bytes"
        if way == "full":
            full_outs = outs
        prop = [r[1][k] for r in reps for k in range(NF) if r[2][k] == "P"]
        whole = [r[1][k] for r in reps for k in range(1, NF) if r[2][k] != "P"]
        row = {"way": way, "kinds": "".join(kinds), "clip_ms": [round(sum(r[1]), 2) for r in reps],
               "full_frame_ms": med(whole), "full_frame_ms_range": [round(min(whole), 2), round(max(whole), 2)] if whole else None,
               "propagated_frame_ms": med(prop), "propagated_frame_ms_range": [round(min(prop), 2), round(max(prop), 2)] if prop else None,
               "transform_flicker_along_motion": round(scene_flicker(outs), 4),
               "psnr_vs_full_db": [None if np.array_equal(a, b) else round(seq_prop_ref.psnr(a, b), 2) for a, b in zip(outs, full_outs)]}
        if way == "auto":
            probes = [d["probe_ms"] for r in reps for d in r[3] if d["kind"] != 0]
            row["probe_ms"] = med(probes); row["probe_ms_range"] = [round(min(probes), 3), round(max(probes), 3)]
            row["changed_permille"] = [None if d["kind"] == 0 else round(1000 * d["changed"] / d["pixels"], 1) for d in ds]
            row["probe_level_pixels"] = ds[1]["pixels"]
        report["ways"][way] = row
        print(json.dumps(row), flush=True)
if out_path:
    with open(out_path, "w") as fh:
        json.dump(report, fh, indent=1)
