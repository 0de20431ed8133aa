#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.22 (region models: the re-find kernel). One JSON line per measurement. Needs a GPU.

    python scripts/region_refind_times.py [--reps 20] [--batches 5]

The re-find kernel alone (k_region_refind, SPEC §6.17 rules R1 to R3) through nct_region_refind_bench: after a warm-up launch, `reps` launches between two HIP events on
the library's stream; median, min and max of `batches` such means. Cases: a 350 x 350 score grid (a 700 x 700 frame at tap 2) to 700 x 700 and to 6000 x 4000 (width x
height: a full-resolution sequence's original size), with a prior and margin 32, and the first also without a prior. Reported beside the time: the bytes the rule must
move — with a prior 2 B per target pixel (one read, one written), 1 B without, plus the grid once — per second, and that rate against the 8 TB/s HBM peak. There is no
pass / fail threshold."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))

HBM_PEAK = 8e12
CASES = (((350, 350), (700, 700), True), ((350, 350), (700, 700), False), ((350, 350), (4000, 6000), True))     # (ht, wt), (H, W), with a prior


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    args = ap.parse_args()
    import nct
    rng = np.random.default_rng(1)
    with nct.Context(0) as c:
        print(json.dumps({"device": c.device_name()}), flush=True)
        for (ht, wt), (H, W), with_prior in CASES:
            # a score as the rule makes it: smooth blobs around 128, so that both branches of R3 are taken
            yy, xx = np.mgrid[0:ht, 0:wt]
            score = np.clip(128 + 90 * np.sin(yy / 23.0) * np.cos(xx / 31.0) + rng.integers(-8, 9, (ht, wt)), 0, 255).astype(np.uint8)
            d_s = c.dev_upload(score)
            d_p = c.dev_upload(rng.integers(0, 256, (H, W)).astype(np.uint8)) if with_prior else None
            d_o = c.dev_alloc(H * W)
            ms = []
            for _ in range(args.batches):
                t = C.c_float(0)
                c._chk(c._l.nct_region_refind_bench(c._h, d_s, ht, wt, d_p, H, W, 32, d_o, args.reps, C.byref(t)))
                ms.append(t.value)
            med = float(np.median(ms))
            moved = H * W * (2 if with_prior else 1) + ht * wt
            print(json.dumps({"pass": "region_refind", "grid": [ht, wt], "target": [H, W], "prior": with_prior, "ms_per_launch": round(med, 5), "min_ms": round(min(ms), 5),
                              "max_ms": round(max(ms), 5), "bytes": moved, "GBps": round(moved / med / 1e6, 1), "of_hbm_peak": round(moved / (med * 1e-3) / HBM_PEAK, 4),
                              "reps": args.reps, "batches": args.batches}), flush=True)
            c.dev_free(d_s); c.dev_free(d_o)
            if d_p is not None:
                c.dev_free(d_p)


if __name__ == "__main__":
    main()
