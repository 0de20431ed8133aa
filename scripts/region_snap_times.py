#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.20 (matte snapping). One JSON line per measurement. Needs a GPU.

    python scripts/region_snap_times.py [--H 4000] [--W 6000] [--ratio 4] [--reps 20] [--batches 5]

The snap alone: nct_region_snap_dev on a matte of H x W bytes (a rectangle) and the 8-bit Lab image of a photograph-like source of that size, at radius 1, 3 and 8
(sigma 10, binary), at W (a multiple of 4: one dword per thread) and, for radius 3, at W - 1 (byte stores): 4 B in and 1 B out per pixel. Beside it, as yardsticks at
the same size: nct_seq_matte_warp_dev (the carry in front of it; 1 B in, 1 B out, a random field in [-3, 3] `ratio` times smaller per side) and
nct_color_finish_upsample_region_dev (the masked finish behind it; 7 B per pixel, a working grid `ratio` times smaller). After a warm-up call of each kind, the wall
time of `reps` enqueued calls between two synchronisations; median, min and max of `batches` such batches. The calls only enqueue, so a batch's time is the device's,
less one launch latency. There is no pass / fail threshold."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=4000)
    ap.add_argument("--W", type=int, default=6000)
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    args = ap.parse_args()
    import nct
    import synth
    from fullres_ref import smooth_ab
    rng = np.random.default_rng(1)
    with nct.Context(0) as c:
        def report(row, t, bpp, H, W):
            med, lo, hi = t
            row.update({"H": H, "W": W, "us_per_call": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "bytes_per_px": bpp,
                        "GBps": round(bpp * H * W / med / 1e3, 1), "reps": args.reps, "batches": args.batches})
            print(json.dumps(row), flush=True)

        H = args.H
        small = synth.image(61, 600, 400)
        for W, radii in ((args.W, (1, 3, 8)), (args.W - 1, (3,))):
            src = c.resize_u8c3(small, H, W)
            matte = np.zeros((H, W), np.uint8); matte[H // 4: 3 * H // 4, W // 3: 5 * W // 6] = 255
            d_m, d_l, d_o = c.dev_upload(matte), c.dev_upload(c.bgr2lab(src)), c.dev_alloc(H * W)
            for r in radii:
                sp = nct.RegionSnapParams.default()
                sp.radius = r
                t = batches(lambda: c._chk(c._l.nct_region_snap_dev(c._h, d_m, d_l, H, W, C.addressof(sp), d_o)), c.synchronize, args.reps, args.batches)
                report({"pass": "region_snap", "radius": r, "sigma": sp.sigma, "binary": sp.binary, "taps": (2 * r + 1) ** 2, "store": "dword" if W % 4 == 0 else "byte"}, t, 5, H, W)
            if W == args.W:
                # the yardsticks: the carry in front of the snap and the masked upsampling finish behind it
                h, w = H // args.ratio, W // args.ratio
                d_f = c.dev_upload(rng.integers(-3, 4, (h, w, 2)).astype(np.int16))
                t = batches(lambda: c._chk(c._l.nct_seq_matte_warp_dev(c._h, d_m, H, W, d_f, h, w, d_o)), c.synchronize, args.reps, args.batches)
                report({"pass": "matte_warp", "field": "random3", "h": h, "w": w}, t, 2, H, W)
                c.dev_free(d_f)
                prm, rg = nct.Params.default(), nct.RegionParams.default()
                d_ab, d_s, d_out = c.dev_upload(smooth_ab(7, h, w).reshape(-1)), c.dev_upload(src), c.dev_alloc(3 * H * W)
                t = batches(lambda: c._chk(c._l.nct_color_finish_upsample_region_dev(c._h, d_ab, h, w, d_s, H, W, d_m, C.addressof(rg), C.addressof(prm), d_out)),
                            c.synchronize, args.reps, args.batches)
                report({"pass": "finish_upsample_region", "mask": "rectangle", "h": h, "w": w}, t, 7, H, W)
                for p in (d_ab, d_s, d_out):
                    c.dev_free(p)
            for p in (d_m, d_l, d_o):
                c.dev_free(p)


if __name__ == "__main__":
    main()
