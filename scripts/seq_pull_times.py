#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.24 (reference region masks in sequences). One JSON line per measurement. Needs a GPU.

    python scripts/seq_pull_times.py [--side 700] [--reps 50] [--batches 5] [--frames 6] [--pkg DIR] [--only kernel|frames]

The hold alone: nct_seq_pull_hold_dev on the five level grids of a side x side frame for K = 2 (one reference unmasked), a field of random vectors in [-3, 3] and a
source mask, all three outputs asked for. After a warm-up call, the wall time of `reps` enqueued calls between two synchronisations; median, min and max of `batches`
such batches — scripts/select_hold_times.py's method, so the figure stands beside k_select_hold's. The bytes are what the rule needs per level pixel: 1 of label, 1 of
pulled mask (the other reference has none), 6 of Lab, 4 of field, 1 of kept mask, 1 of source mask in; 3 out.
Then whole frames at side x side with the synthetic weights: a sequence over one reference with motion on that never sets a reference mask — the path that must not
have changed — the wall time of each nct_seq_frame call in the second round on a warm context, and their median; and the same sequence with a half mask on the
reference. --pkg names another build's python directory (its nct package beside its lib/), to time the first of the two on that build; --only picks one part."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def hold_alone(c, args):
    import seq_refregion_ref as srr
    sizes = []
    h = w = args.side
    for _ in range(5):
        sizes.insert(0, (h, w)); h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    K = 2
    for l, (h, w) in enumerate(sizes):
        case = srr.hold_case(h, w, K, 11 + l, "random", True, unmasked=1)
        dp = [None if p is None else c.dev_upload(p) for p in case["pulled"]]
        ins = [c.dev_upload(case[k]) for k in ("label", "prev", "lab", "lab_prev", "field", "src_mask")]
        outs = [c.dev_alloc(h * w) for _ in range(3)]
        pp = (C.c_void_p * K)(*dp)
        call = lambda: c._chk(c._l.nct_seq_pull_hold_dev(c._h, pp, K, ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], h, w, 0.7, 10.0, outs[0], outs[1], outs[2]))
        med, lo, hi = batches(call, c.synchronize, args.reps, args.batches)
        nbytes = (1 + 1 + 6 + 4 + 1 + 1 + 3) * h * w
        print(json.dumps({"pass": "seq_pull_hold", "K": K, "level": l, "h": h, "w": w, "us_per_call": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2),
                          "MB": round(nbytes / 1e6, 2), "GBps": round(nbytes / med / 1e3, 1), "reps": args.reps, "batches": args.batches}), flush=True)
        c.synchronize()
        for p in [q for q in dp if q is not None] + ins + outs:
            c.dev_free(p)


def whole_frames(c, args, masked):
    import region_ref
    import seq_ref
    import synth
    from caffemodel_io import synthetic_vgg19
    c.vgg19_load_raw(*synthetic_vgg19(19))
    side = args.side
    ref = synth.image(1001, side, side)
    frames = seq_ref.static_frames(args.frames, side, side)
    for rep in range(2):                                                   # the first round warms the arena and the code objects up
        c.seq_begin(ref, frames[0].shape)
        c.seq_set_motion()
        if masked:
            c.seq_set_ref_region(0, region_ref.mask("half", side, side))
        ms = []
        for f in frames:
            t0 = time.perf_counter(); c.seq_frame(f); ms.append((time.perf_counter() - t0) * 1e3)
        c.seq_end()
        print(json.dumps({"pass": "frames", "round": rep, "side": side, "K": 1, "ref_mask": bool(masked), "build": args.pkg or "this tree",
                          "seq_frame_ms": [round(x, 2) for x in ms], "median_blended_ms": round(float(np.median(ms[1:])), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--only", choices=("kernel", "frames"), default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, args.pkg or os.path.join(REPO, "neural-color-transfer_amd", "python"))
    import nct
    if args.only != "frames" and not args.pkg:
        with nct.Context(0) as c:
            hold_alone(c, args)
    if args.only != "kernel":
        with nct.Context(0) as c:
            whole_frames(c, args, False)
        if not args.pkg:
            with nct.Context(0) as c:
                whole_frames(c, args, True)


if __name__ == "__main__":
    main()
