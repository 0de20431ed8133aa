#!/usr/bin/env python3
"""Times of the look-up table calls on device-resident images: nct_lut_fit_dev and nct_lut_apply_dev at 700 x 700 and 6000 x 4000 for
N = 17, 33, 65, wall time of `reps` enqueued calls between two synchronisations; and the table against full-resolution output: a 6000 x 4000 source, the table
fitted from its working-size pair (nct_pair_fit_lut) and applied to the original, compared with nct_process_pair_fullres, every call warmed once and then timed three times. One JSON line per measurement.
Per-kernel times come from a run of this script under `rocprofv3 --kernel-trace --stats -- python scripts/lut_times.py --reps 3 --no-fullres`.

    python scripts/lut_times.py [--reps 10] [--no-fullres]
"""
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


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def main():
    import nct
    import synth
    from caffemodel_io import synthetic_vgg19
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-fullres", action="store_true")
    args = ap.parse_args()
    ws, bs = synthetic_vgg19(19)
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        ref = synth.image(62, 800, 640)
        small = synth.image(61, 600, 400)
        for h, w in ((700, 700), (6000, 4000)):
            src = c.resize_u8c3(small, h, w)
            # a graded look as the result: the pair's own result at 700 x 700, a smooth per-channel curve of the source at 24 MP (the splat's cost depends on the
            # source's colours only)
            res = c.process_pair(src, ref) if h <= 1000 else np.clip(src.astype(np.float32) * [0.8, 1.05, 1.2] + [20, -5, 8], 0, 255).astype(np.uint8)
            npix = h * w
            d_s, d_o, d_out = c.dev_upload(src), c.dev_upload(res), c.dev_alloc(3 * npix)
            for N in (17, 33, 65):
                prm = nct._lut_params(N, None)
                d_lut = c.dev_alloc(12 * N ** 3)
                for name, call in (("fit", lambda: c._chk(c._l.nct_lut_fit_dev(c._h, d_s, d_o, npix, C.addressof(prm), d_lut, None))),
                                   ("apply", lambda: c._chk(c._l.nct_lut_apply_dev(c._h, d_lut, N, d_s, npix, d_out)))):
                    call(); c.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        call()
                    c.synchronize()
                    us = (time.perf_counter() - t0) / args.reps * 1e6
                    row = {"call": name, "h": h, "w": w, "N": N, "us_per_call": round(us, 1), "reps": args.reps}
                    if name == "apply":
                        row["GB_per_s_of_6B_per_pixel"] = round(6.0 * npix / us / 1e3, 1)
                    print(json.dumps(row), flush=True)
                c.synchronize(); c.dev_free(d_lut)
            c.synchronize()
            for p in (d_s, d_o, d_out):
                c.dev_free(p)
        if not args.no_fullres:
            src0 = c.resize_u8c3(small, 6000, 4000)
            wh, ww = nct.working_size(6000, 4000, 1000)

            def timed(fn, reps=3):
                """the call's result and its wall times in ms: one warm-up call, then `reps` timed ones"""
                out, ms = fn(), []
                for _ in range(reps):
                    t0 = time.perf_counter(); out = fn(); ms.append(round((time.perf_counter() - t0) * 1e3, 2))
                return out, ms
            full, t_full = timed(lambda: c.process_pair_fullres(src0, ref, 1000))
            work = c.resize_u8c3(src0, wh, ww)
            _, t_pair = timed(lambda: c.process_pair(work, ref))
            d_src0, d_out0 = c.dev_upload(src0), c.dev_alloc(3 * 6000 * 4000)
            for N in (17, 33, 65):
                lut, t_fit = timed(lambda: c.pair_fit_lut(N))
                out, t_apply = timed(lambda: c.lut_apply(lut, src0))
                d_lut = c.dev_upload(lut)
                _, t_dev = timed(lambda: (c._chk(c._l.nct_lut_apply_dev(c._h, d_lut, N, d_src0, 6000 * 4000, d_out0)), c.synchronize()))
                c.dev_free(d_lut)
                print(json.dumps({"fullres_vs_lut": "6000x4000", "N": N, "psnr_lut_vs_fullres_dB": round(psnr(out, full), 2), "psnr_source_vs_fullres_dB": round(psnr(src0, full), 2),
                                  "ms_fullres_call": t_full, "ms_working_size_pair": t_pair, "ms_pair_fit_lut": t_fit,
                                  "ms_lut_apply_host_call_with_copies": t_apply, "ms_lut_apply_dev_call": t_dev}), flush=True)
            c.synchronize()
            for p in (d_src0, d_out0):
                c.dev_free(p)

if __name__ == "__main__":
    main()
