#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.19 (region tracking). One JSON line per measurement. Needs a GPU.

    python scripts/matte_warp_times.py [--H 4000] [--W 6000] [--ratio 4] [--reps 20] [--batches 5] [--side 700]

The carry alone: nct_seq_matte_warp_dev on a target of H x W bytes from a field `ratio` times smaller per side, under a zero field, a constant one and random
vectors in [-3, 3] (a gather that stays near the pixel), at W (a multiple of 4: one dword per thread) and at W - 1 (byte stores). After a warm-up call, the wall
time of `reps` enqueued calls between two synchronisations; median, min and max of `batches` such batches. The calls only enqueue, so a batch's time is the device's,
less one launch latency. Beside them the floor: a device-to-device copy of the same H * W bytes, 1 B in and 1 B out per pixel, timed the same way.
Then whole frames at side x side: a tracked sequence (a matte on frame 0, plan F B P B P, motion on) against the same frames with the carried matte set explicitly
before every frame, per frame the wall time of the frame call and its other_ms."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))


def batches(call, sync, reps, n):
    call(); sync()                                                         # warm-up
    us = []
    for _ in range(n):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        us.append((time.perf_counter() - t0) / reps * 1e6)
    return float(np.median(us)), min(us), max(us)


def carry_alone(c, args):
    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):      # the runtime the library is linked against, already loaded with it
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            pass
    if hip is None:
        raise RuntimeError("the HIP runtime library was not found")
    rng = np.random.default_rng(1)
    for W in (args.W, args.W - 1):
        H = args.H
        h, w = H // args.ratio, W // args.ratio
        fields = {"zero": np.zeros((h, w, 2), np.int16), "constant": np.full((h, w, 2), 1, np.int16), "random3": rng.integers(-3, 4, (h, w, 2)).astype(np.int16)}
        d_m, d_o = c.dev_upload(rng.integers(0, 256, (H, W), dtype=np.uint8)), c.dev_alloc(H * W)
        for name, f in fields.items():
            d_f = c.dev_upload(f)
            med, lo, hi = batches(lambda: c._chk(c._l.nct_seq_matte_warp_dev(c._h, d_m, H, W, d_f, h, w, d_o)), c.synchronize, args.reps, args.batches)
            print(json.dumps({"pass": "matte_warp", "field": name, "H": H, "W": W, "h": h, "w": w, "store": "dword" if W % 4 == 0 else "byte", "us_per_call": round(med, 1),
                              "min_us": round(lo, 1), "max_us": round(hi, 1), "GBps_1in_1out": round(2 * H * W / med / 1e3, 1), "reps": args.reps, "batches": args.batches}), flush=True)
            c.synchronize(); c.dev_free(d_f)
        c.dev_free(d_m); c.dev_free(d_o)
        # the floor: the runtime's own device-to-device copy between two arena blocks, enqueued on the null stream
        d_a, d_b = c.dev_upload(rng.integers(0, 256, (H, W), dtype=np.uint8)), c.dev_alloc(H * W)
        c.synchronize()

        def copy():
            if hip.hipMemcpyAsync(C.c_void_p(d_b), C.c_void_p(d_a), C.c_size_t(H * W), 3, None) != 0:      # 3: hipMemcpyDeviceToDevice
                raise RuntimeError("hipMemcpyAsync failed")

        def sync():
            if hip.hipStreamSynchronize(None) != 0:
                raise RuntimeError("hipStreamSynchronize failed")
        med, lo, hi = batches(copy, sync, args.reps, args.batches)
        print(json.dumps({"pass": "d2d_copy", "H": H, "W": W, "us_per_call": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                          "GBps_1in_1out": round(2 * H * W / med / 1e3, 1), "reps": args.reps, "batches": args.batches}), flush=True)
        c.dev_free(d_a); c.dev_free(d_b)


def frames_at(c, args):
    import nct
    import seq_ref
    import synth
    from caffemodel_io import synthetic_vgg19
    S, kinds = args.side, "FBPBP"
    c.vgg19_load_raw(*synthetic_vgg19(19))
    frames = seq_ref.pan_frames(len(kinds), S, S, step=4)
    ref = synth.image(2000, S, S)
    matte = np.zeros((S, S), np.uint8); matte[S // 4: 3 * S // 4, S // 3: 5 * S // 6] = 255

    def run(mattes, tracking):
        c.seq_begin(ref, (S, S, 3), nct.Params.default())
        try:
            c.seq_set_motion(3, 1, 1)
            c.seq_set_region_tracking(tracking)
            rows = []
            for t, (f, k) in enumerate(zip(frames, kinds)):
                set_ms = 0.0
                if mattes[t] is not None:
                    t0 = time.perf_counter(); c.seq_set_region(mattes[t]); set_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                _, tm = c.seq_frame_propagate(f, want_timing=True) if k == "P" else c.seq_frame(f, want_timing=True)
                rows.append({"kind": k, "frame_ms": (time.perf_counter() - t0) * 1e3, "other_ms": tm["other_ms"], "set_region_ms": set_ms, "matte": c.seq_get_region()[0]})
            return rows
        finally:
            c.seq_end()
    run([matte] + [None] * (len(kinds) - 1), True)                        # warm-up: the arena and the kernels
    tracked = run([matte] + [None] * (len(kinds) - 1), True)
    explicit = run([r["matte"] for r in tracked], False)
    for t, (a, b) in enumerate(zip(tracked, explicit)):
        assert np.array_equal(a["matte"], b["matte"])
        print(json.dumps({"pass": "frame", "side": S, "t": t, "kind": a["kind"], "moved_px": int((a["matte"] != matte).sum()),
                          "tracked_frame_ms": round(a["frame_ms"], 2), "tracked_other_ms": round(a["other_ms"], 3),
                          "explicit_frame_ms": round(b["frame_ms"], 2), "explicit_other_ms": round(b["other_ms"], 3), "explicit_set_region_ms": round(b["set_region_ms"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=4000)
    ap.add_argument("--W", type=int, default=6000)
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--side", type=int, default=700)
    args = ap.parse_args()
    import nct
    with nct.Context(0) as c:
        carry_alone(c, args)
        frames_at(c, args)


if __name__ == "__main__":
    main()
