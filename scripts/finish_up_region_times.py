#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.18 (the masked upsampling finish). One JSON line per measurement. Needs a GPU.

    python scripts/finish_up_region_times.py [--mp 24] [--ratio 4] [--reps 20] [--batches 5]

A target of `mp` megapixels (3 : 2) and a working grid `ratio` times smaller per side. Per call, on device pointers: nct_color_finish_upsample_dev and
nct_color_finish_guided_dev (the unmasked passes, 6 B per original pixel) beside nct_color_finish_upsample_region_dev and nct_color_finish_guided_region_dev
(7 B per original pixel) under three masks — a ramp (every byte value: kept and converted pixels share wavefronts), all 255 (every pixel converted: the unmasked
pass plus the mask byte) and all 0 with protect = 1 (every pixel kept: no Lab -> BGR at all). After a warm-up call of each kind, the wall time of `reps` enqueued
calls between two synchronisations; the median of `batches` such batches. The calls only enqueue, so a batch's time is the device's, less one launch latency."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mp", type=int, default=24)
    ap.add_argument("--ratio", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    args = ap.parse_args()
    import nct
    import synth
    from fullres_ref import smooth_ab
    H = int(round((args.mp * 1e6 / 1.5) ** 0.5)); W = H * 3 // 2
    h, w = H // args.ratio, W // args.ratio
    ab = smooth_ab(7, h, w)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = {"ramp": (xx * 256 // W).astype(np.uint8), "all255": np.full((H, W), 255, np.uint8), "all0_protect": np.zeros((H, W), np.uint8)}
    with nct.Context(0) as c:
        src = c.resize_u8c3(synth.image(61, 600, 400), H, W)
        lab_w = c.bgr2lab(c.resize_u8c3(src, h, w))
        prm, gp = nct.Params.default(), nct.GuidedParams.default()
        rg = [nct.RegionParams.default(), nct.RegionParams.default()]
        rg[1].protect = 1
        d_ab, d_lw, d_s, d_o = c.dev_upload(ab.reshape(-1)), c.dev_upload(lab_w), c.dev_upload(src), c.dev_alloc(3 * H * W)
        d_m = {k: c.dev_upload(m) for k, m in masks.items()}
        P, G = C.addressof(prm), C.addressof(gp)
        calls = {("upsample", None): lambda: c._l.nct_color_finish_upsample_dev(c._h, d_ab, h, w, d_s, H, W, P, d_o),
                 ("guided", None): lambda: c._l.nct_color_finish_guided_dev(c._h, d_ab, d_lw, h, w, d_s, H, W, G, P, d_o)}
        for k in masks:
            R = C.addressof(rg[1 if k == "all0_protect" else 0])
            calls[("upsample", k)] = lambda k=k, R=R: c._l.nct_color_finish_upsample_region_dev(c._h, d_ab, h, w, d_s, H, W, d_m[k], R, P, d_o)
            calls[("guided", k)] = lambda k=k, R=R: c._l.nct_color_finish_guided_region_dev(c._h, d_ab, d_lw, h, w, d_s, H, W, d_m[k], R, G, P, d_o)
        for (kind, mask), call in calls.items():
            c._chk(call()); c.synchronize()                                # warm-up
            us = []
            for _ in range(args.batches):
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    c._chk(call())
                c.synchronize()
                us.append((time.perf_counter() - t0) / args.reps * 1e6)
            med = float(np.median(us))
            bpp = 6 if mask is None else 7
            print(json.dumps({"pass": kind, "mask": mask, "H": H, "W": W, "h": h, "w": w, "us_per_call": round(med, 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
                              "bytes_per_px": bpp, "GBps": round(bpp * H * W / med / 1e3, 1), "reps": args.reps, "batches": args.batches}), flush=True)
        for p in [d_ab, d_lw, d_s, d_o] + list(d_m.values()):
            c.dev_free(p)


if __name__ == "__main__":
    main()
