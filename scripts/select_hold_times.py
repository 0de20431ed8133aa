#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.23 (sequences over several references). One JSON line per measurement. Needs a GPU.

    python scripts/select_hold_times.py [--side 700] [--reps 50] [--batches 5] [--frames 4]

The selection alone: nct_select_reference_hold_dev on the five level grids of a side x side frame for K = 2 and K = 4, with a field of random vectors in [-3, 3], and
beside it nct_select_reference_dev on the same maps. After a warm-up call, the wall time of `reps` enqueued calls between two synchronisations; median, min and max of
`batches` such batches. The calls only enqueue, so a batch's time is the device's, less one launch latency. The bytes are what the rule needs per level pixel: 4 K of
error words, 6 of Lab, 4 of field, 1 of kept label and 3 of the selected guidance image in; 1 + 3 + 4 out.
Then whole frames at side x side with the synthetic weights: a K = 2 sequence with motion on (a first frame, then held frames) against nct_process_multi of the same
images, the wall time of each call; and, on contexts of their own, the arena bytes a context holds after the frames of that sequence and of the sequence over
its first reference alone."""
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


def selection_alone(c, args):
    import seq_multi_ref as smr
    sizes = []
    h = w = args.side
    for _ in range(5):
        sizes.insert(0, (h, w)); h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for K in (2, 4):
        for l, (h, w) in enumerate(sizes):
            case = smr.hold_case(h, w, K, 7 * K + l)
            de = [c.dev_upload(e) for e in case["errs"]]
            dg = [c.dev_upload(g) for g in case["guides"]]
            ins = [c.dev_upload(case[k]) for k in ("prev_label", "lab", "lab_prev", "field")]
            outs = [c.dev_alloc(h * w), c.dev_alloc(3 * h * w), c.dev_alloc(4 * h * w)]
            ep, gp = (C.c_void_p * K)(*de), (C.c_void_p * K)(*dg)
            hold = lambda: c._chk(c._l.nct_select_reference_hold_dev(c._h, ep, gp, K, h, w, ins[0], ins[1], ins[2], ins[3], 0.005, 10.0, outs[0], outs[1], outs[2], None, None))
            plain = lambda: c._chk(c._l.nct_select_reference_dev(c._h, ep, gp, K, h, w, outs[0], outs[1], outs[2]))
            for name, call, nbytes in (("select_hold", hold, (4 * K + 6 + 4 + 1 + 3 + 8) * h * w), ("select_reference", plain, (4 * K + 3 + 8) * h * w)):
                med, lo, hi = batches(call, c.synchronize, args.reps, args.batches)
                print(json.dumps({"pass": name, "K": K, "level": l, "h": h, "w": w, "us_per_call": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2),
                                  "MB": round(nbytes / 1e6, 2), "GBps": round(nbytes / med / 1e3, 1), "reps": args.reps, "batches": args.batches}), flush=True)
            c.synchronize()
            for p in de + dg + ins + outs:
                c.dev_free(p)


def whole_frames(c, nct, args):
    import seq_multi_ref as smr
    import seq_ref
    import synth
    from caffemodel_io import synthetic_vgg19
    c.vgg19_load_raw(*synthetic_vgg19(19))
    side = args.side
    a = synth.image(1001, side, side)
    refs = [a, smr.competing(a)]
    frames = seq_ref.static_frames(args.frames, side, side)
    for rep in range(2):                                                   # the first round warms the arena and the code objects up
        multi = []
        for f in frames:
            t0 = time.perf_counter(); c.process_multi(f, refs); multi.append((time.perf_counter() - t0) * 1e3)
        c.seq_begin_multi(refs, frames[0].shape)
        c.seq_set_motion()
        seq = []
        for f in frames:
            t0 = time.perf_counter(); c.seq_frame(f); seq.append((time.perf_counter() - t0) * 1e3)
        c.seq_end()
        print(json.dumps({"pass": "frames", "round": rep, "side": side, "K": 2, "process_multi_ms": [round(x, 2) for x in multi], "seq_frame_ms": [round(x, 2) for x in seq]}), flush=True)


def arena_bytes(nct, args):
    import seq_multi_ref as smr
    import seq_ref
    import synth
    from caffemodel_io import synthetic_vgg19
    a = synth.image(1001, args.side, args.side)
    frames = seq_ref.static_frames(2, args.side, args.side)
    for refs in ([a], [a, smr.competing(a)]):
        with nct.Context(0) as c:
            c.vgg19_load_raw(*synthetic_vgg19(19))
            c.seq_begin_multi(refs, frames[0].shape)
            opened = c.counter(nct.CTR_ARENA_BYTES)
            c.seq_set_motion()
            for f in frames:
                c.seq_frame(f)
            print(json.dumps({"pass": "arena", "side": args.side, "K": len(refs), "bytes_after_begin": opened, "bytes_after_frames": c.counter(nct.CTR_ARENA_BYTES)}), flush=True)
            c.seq_end()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    args = ap.parse_args()
    import nct
    with nct.Context(0) as c:
        selection_alone(c, args)
    with nct.Context(0) as c:
        whole_frames(c, nct, args)
    arena_bytes(nct, args)


if __name__ == "__main__":
    main()
