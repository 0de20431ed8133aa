#!/usr/bin/env python3
"""Times of the 16-bit table apply and of the shot accumulator on device-resident images. nct_lut_apply_u16_dev and nct_lut_apply_dev on the same
24 MP (6000 x 4000) at N = 17 and 33, the two alternating in one session: after a warm-up call the wall time of `reps` enqueued calls between two synchronisations,
median (min ... max) of `batches` such batches. Then, on a context that has run a 700 x 700 pair: nct_pair_fit_lut at N = 33 beside one nct_lut_accum_add_run and one
nct_lut_accum_solve_dev, each call ending in a synchronise, median of `batches`. One JSON line per measurement, also appended to --out.

    python scripts/lut16_times.py [--reps 20] [--batches 7] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))


def main():
    import nct
    import synth
    from caffemodel_io import synthetic_vgg19
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n"); sink.flush()

    def stats(v):
        return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}

    ws, bs = synthetic_vgg19(19)
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        small, ref = synth.image(61, 600, 400), synth.image(62, 800, 640)
        h, w = 6000, 4000
        npix = h * w
        src8 = c.resize_u8c3(small, h, w)
        src16 = src8.astype(np.uint16) * 257 ^ np.random.default_rng(1).integers(0, 256, src8.shape).astype(np.uint16)            # both bytes in use
        d8, d16, o8, o16 = c.dev_upload(src8), c.dev_upload(src16), c.dev_alloc(3 * npix), c.dev_alloc(6 * npix)
        look = c.resize_u8c3(np.clip(small.astype(np.float32) * [0.8, 1.05, 1.2] + [20, -5, 8], 0, 255).astype(np.uint8), h, w)
        for N in (17, 33):
            d_lut = c.dev_upload(c.lut_fit(src8[::8, ::8], look[::8, ::8], N))
            calls = {"lut_apply_u16_dev": (lambda: c._chk(c._l.nct_lut_apply_u16_dev(c._h, d_lut, N, d16, npix, o16)), 12.0),
                     "lut_apply_dev": (lambda: c._chk(c._l.nct_lut_apply_dev(c._h, d_lut, N, d8, npix, o8)), 6.0)}
            us = {k: [] for k in calls}
            for call, _ in calls.values():
                call()
            c.synchronize()
            for _ in range(args.batches):                    # the two alternate, batch by batch
                for name, (call, _) in calls.items():
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        call()
                    c.synchronize()
                    us[name].append((time.perf_counter() - t0) / args.reps * 1e6)
            for name, (_, bytes_per_pixel) in calls.items():
                med = statistics.median(us[name])
                emit({"call": name, "h": h, "w": w, "N": N, "us_per_call": stats(us[name]), "reps": args.reps, "batches": args.batches,
                      "bytes_per_pixel": bytes_per_pixel, "TB_per_s": round(bytes_per_pixel * npix / med / 1e6, 3)})
            c.synchronize(); c.dev_free(d_lut)
        c.synchronize()
        for p in (d8, d16, o8, o16):
            c.dev_free(p)
        # the shot accumulator beside nct_pair_fit_lut, N = 33, after a 700 x 700 pair
        src = c.resize_u8c3(small, 700, 700)
        c.process_pair(src, ref)
        N = 33
        d_lut = c.dev_alloc(12 * N ** 3)
        lam = nct.LutParams.default().lambda_

        def timed(fn):
            fn(); c.synchronize()
            out = []
            for _ in range(args.batches):
                t0 = time.perf_counter(); fn(); c.synchronize(); out.append((time.perf_counter() - t0) * 1e6)
            return stats(out)
        emit({"call": "pair_fit_lut", "h": 700, "w": 700, "N": N, "us_per_call": timed(lambda: c.pair_fit_lut(N))})
        c.lut_accum_begin(N)
        emit({"call": "lut_accum_add_run", "h": 700, "w": 700, "N": N, "us_per_call": timed(c.lut_accum_add_run)})
        emit({"call": "lut_accum_solve_dev", "N": N, "adds": c.lut_accum_info()["adds"],
              "us_per_call": timed(lambda: c._chk(c._l.nct_lut_accum_solve_dev(c._h, lam, d_lut, None)))})
        c.lut_accum_end()
        c.synchronize(); c.dev_free(d_lut)


if __name__ == "__main__":
    main()
