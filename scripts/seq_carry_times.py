#!/usr/bin/env python3
"""Speed and quality of the correspondence carry on an MI355X. One JSON line per measurement, also appended to --out.

Eight 700 x 700 frames of the 16 px / frame pan of §3.10 (seq_ref.pan_frames) and of the static noisy scene (seq_ref.static_frames), reference synth.image(2000, 640,
800), synthetic weights, tau = 0.7, motion 3 / 1 / 1. Per scene: the carry off, then carry_iters 10, 6, 4, 2, 1. Each configuration runs the eight frames `batches`
times (a warm-up sequence first); per frame after the first the median (min ... max) over the batches of total_ms, patchmatch_ms and pm_level_ms[l] of the library's
stage clock. The moves and the merge have no clock of their own: their time per level is pm_level_ms of carry_iters = 10 minus the carry-off sequence's, the same
PatchMatch launches on both sides. From one more sequence with the level report: PSNR of every frame against the carry-off sequence, the transform flicker (along the
pan where the scene pans), and the finest level's mean distance of the last frame.

--package DIR measures another build of the package (its python/ and lib/, for instance the parent commit's, built beside this one) in the same session; such a
build may lack the carry, so only the carry-off sequence runs on it (--off-only).

    python scripts/seq_carry_times.py [--frames 8] [--size 700] [--batches 7] [--package DIR --off-only] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
PACKAGE = os.path.join(REPO, "neural-color-transfer_amd")
if "--package" in sys.argv:
    PACKAGE = os.path.abspath(sys.argv[sys.argv.index("--package") + 1])
    os.environ["NCT_LIB"] = os.path.join(PACKAGE, "lib", "libnct.so")
sys.path.insert(0, os.path.join(PACKAGE, "python"))
MOT = (3, 1, 1)
STEP = 16
CONFIGS = (None, 10, 6, 4, 2, 1)


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def run(c, nct, ref, frames, carry, levels_report=False):
    """one sequence -> per frame (result, timing dict, finest-level mean distance or None)"""
    c.seq_begin(ref, frames[0].shape)
    try:
        c.seq_set_motion(*MOT)
        if carry is not None:
            c.seq_set_carry(True, carry)
        out = []
        for f in frames:
            if levels_report:
                o, lv = c.seq_frame_levels(f, want_color=False)
                out.append((o, lv["timing"], float(np.mean(lv["annd"][4]))))
            else:
                o, tm = c.seq_frame(f, want_timing=True)
                out.append((o, tm, None))
        return out
    finally:
        c.seq_end()


def main():
    import nct
    import seq_mc_ref
    import seq_ref
    import synth
    from caffemodel_io import synthetic_vgg19
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=700)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--package", default=None)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    n, s = args.frames, args.size
    scenes = {"pan": seq_ref.pan_frames(n, s, s, step=STEP), "static": seq_ref.static_frames(n, s, s)}
    ref = synth.image(2000, 640, 800)
    ws, bs = synthetic_vgg19(19)
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        for scene, frames in scenes.items():
            base = off_levels = None
            run(c, nct, ref, frames[:2], None)                              # warm-up
            for carry in (CONFIGS[:1] if args.off_only else CONFIGS):
                per = {k: [[] for _ in range(n)] for k in ("total_ms", "patchmatch_ms")}
                lvl = [[[] for _ in range(5)] for _ in range(n)]
                for _ in range(args.batches):
                    for t, (_, tm, _) in enumerate(run(c, nct, ref, frames, carry)):
                        for k in per:
                            per[k][t].append(tm[k])
                        for l in range(5):
                            lvl[t][l].append(tm["pm_level_ms"][l])
                rep = run(c, nct, ref, frames, carry, levels_report=True)
                outs = [o for o, _, _ in rep]
                if carry is None:
                    base = outs
                    off_levels = [statistics.median([statistics.median(lvl[t][l]) for t in range(1, n)]) for l in range(5)]
                later = lambda key: stats([statistics.median(per[key][t]) for t in range(1, n)])
                pm_levels = [round(statistics.median([statistics.median(lvl[t][l]) for t in range(1, n)]), 3) for l in range(5)]
                row = {"package": os.path.relpath(PACKAGE, REPO), "scene": scene, "size": s, "frames": n, "batches": args.batches, "carry_iters": carry, "first_frame_total_ms": stats(per["total_ms"][0]),
                       "later_frames_total_ms": later("total_ms"), "later_frames_patchmatch_ms": later("patchmatch_ms"), "later_frames_pm_level_ms": pm_levels,
                       "pm_level_launches": rep[-1][1]["pm_level_launches"], "psnr_vs_carry_off_dB": [round(psnr(a, b), 2) for a, b in zip(outs, base)],
                       "finest_mean_distance_last_frame": round(rep[-1][2], 5)}
                if scene == "pan":
                    row["flicker_along_pan"], row["transform_flicker_along_pan"] = (round(v, 4) for v in seq_mc_ref.warped_flicker(outs, frames, STEP))
                else:
                    row["flicker"], row["transform_flicker"] = round(seq_ref.flicker(outs), 4), round(seq_ref.transform_flicker(outs, frames), 4)
                if carry == 10:
                    row["moves_and_merge_ms_per_level"] = [round(a - b, 3) for a, b in zip(pm_levels, off_levels)]
                emit(row)


if __name__ == "__main__":
    main()
