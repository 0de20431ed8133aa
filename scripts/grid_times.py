#!/usr/bin/env python3
"""Speed and quality of the local colour grids on an MI355X. One JSON line per measurement, also appended to --out.

speed: nct_grid_apply_dev and nct_grid_apply_u16_dev on device-resident 24 MP (6000 x 4000) with 16 x 16 x 16 and 32 x 32 x 16 grids, beside nct_lut_apply_dev and
nct_lut_apply_u16_dev (N = 33) in the same session, the calls alternating batch by batch: after a warm-up call the wall time of `reps` enqueued calls between two
synchronisations, median (min ... max) of `batches` such batches (§3.25's method). Then one nct_grid_fit_dev at 700 x 700 and at 24 MP and, on a context that has run a
700 x 700 pair, nct_pair_fit_grid beside nct_pair_fit_lut, each call ending in a synchronise.

quality: a 24 MP original (the demo photograph in0 enlarged where tests/golden/natural holds it, else its committed stand-in), the grid fitted from the working-size
run (nct_pair_fit_grid) and applied to the original; PSNR against nct_process_pair_fullres (the exact finish), beside the table (N = 33), the upsampling finish and
the guided one. lambda in {1, 4, 16, 64, 256} times the spatial size in {8, 16, 32} (longer side; the shorter in proportion, 16 along luma), and the same sweep on the
two-gradings fixture of tests/grid_ref.py (mean absolute error).

    python scripts/grid_times.py [speed] [quality] [--reps 20] [--batches 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))
LAMBDAS = (1.0, 4.0, 16.0, 64.0, 256.0)
SIZES = (8, 16, 32)


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float32) - b.astype(np.float32)) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def stats(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def grid_shape(h, w, G):
    lng, sht = max(h, w), min(h, w)
    other = max(2, (2 * G * sht + lng) // (2 * lng))
    return (G, other, 16) if h >= w else (other, G, 16)


def speed(c, nct, synth, args, emit):
    small, ref = synth.image(61, 600, 400), synth.image(62, 800, 640)
    h, w = 6000, 4000
    npix = h * w
    src8 = c.resize_u8c3(small, h, w)
    src16 = src8.astype(np.uint16) * 257 ^ np.random.default_rng(1).integers(0, 256, src8.shape).astype(np.uint16)            # both bytes in use
    look = c.resize_u8c3(np.clip(small.astype(np.float32) * [0.8, 1.05, 1.2] + [20, -5, 8], 0, 255).astype(np.uint8), h, w)
    d8, d16, o8, o16 = c.dev_upload(src8), c.dev_upload(src16), c.dev_alloc(3 * npix), c.dev_alloc(6 * npix)
    N = 33
    d_lut = c.dev_upload(c.lut_fit(src8[::8, ::8], look[::8, ::8], N))
    for g in ((16, 16, 16), (32, 32, 16)):
        d_grid = c.dev_upload(c.grid_fit(src8[::8, ::8], look[::8, ::8], g))
        calls = {"grid_apply_u16_dev": (lambda: c._chk(c._l.nct_grid_apply_u16_dev(c._h, d_grid, *g, d16, h, w, o16)), 12.0),
                 "lut_apply_u16_dev": (lambda: c._chk(c._l.nct_lut_apply_u16_dev(c._h, d_lut, N, d16, npix, o16)), 12.0),
                 "grid_apply_dev": (lambda: c._chk(c._l.nct_grid_apply_dev(c._h, d_grid, *g, d8, h, w, o8)), 6.0),
                 "lut_apply_dev": (lambda: c._chk(c._l.nct_lut_apply_dev(c._h, d_lut, N, d8, npix, o8)), 6.0)}
        us = {k: [] for k in calls}
        for call, _ in calls.values():
            call()
        c.synchronize()
        for _ in range(args.batches):                    # the four alternate, batch by batch
            for name, (call, _) in calls.items():
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    call()
                c.synchronize()
                us[name].append((time.perf_counter() - t0) / args.reps * 1e6)
        for name, (_, bpp) in calls.items():
            med = statistics.median(us[name])
            emit({"call": name, "h": h, "w": w, "grid": list(g) if name.startswith("grid") else None, "N": None if name.startswith("grid") else N,
                  "us_per_call": stats(us[name]), "reps": args.reps, "batches": args.batches, "bytes_per_pixel": bpp, "TB_per_s": round(bpp * npix / med / 1e6, 3)})
        c.synchronize(); c.dev_free(d_grid)

    def timed(fn):
        fn(); c.synchronize()
        out = []
        for _ in range(args.batches):
            t0 = time.perf_counter(); fn(); c.synchronize(); out.append((time.perf_counter() - t0) * 1e6)
        return stats(out)
    prm = nct.GridParams.default()
    d_x = c.dev_alloc(8 * 12 * 16 ** 3)
    import ctypes as C
    emit({"call": "grid_fit_dev", "h": h, "w": w, "grid": [16, 16, 16],
          "us_per_call": timed(lambda: c._chk(c._l.nct_grid_fit_dev(c._h, d8, o8, h, w, C.addressof(prm), d_x, None)))})
    d7, o7 = c.dev_upload(c.resize_u8c3(small, 700, 700)), c.dev_upload(c.resize_u8c3(look[::8, ::8], 700, 700))
    emit({"call": "grid_fit_dev", "h": 700, "w": 700, "grid": [16, 16, 16],
          "us_per_call": timed(lambda: c._chk(c._l.nct_grid_fit_dev(c._h, d7, o7, 700, 700, C.addressof(prm), d_x, None)))})
    c.synchronize()
    for p in (d8, d16, o8, o16, d_lut, d_x, d7, o7):
        c.dev_free(p)
    c.process_pair(c.resize_u8c3(small, 700, 700), ref)
    emit({"call": "pair_fit_grid", "h": 700, "w": 700, "grid": [16, 16, 16], "us_per_call": timed(lambda: c.pair_fit_grid())})
    emit({"call": "pair_fit_lut", "h": 700, "w": 700, "N": N, "us_per_call": timed(lambda: c.pair_fit_lut(N))})


def quality(c, nct, synth, args, emit):
    import grid_ref
    import natural_inputs
    from PIL import Image
    natural = natural_inputs.present()
    d = natural_inputs.DIR if natural else natural_inputs.require()
    load = lambda n: np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, n + ".png")).convert("RGB"))[..., ::-1])
    small, ref = load("in0"), load("tar0")
    k = 6000.0 / max(small.shape[:2])
    H, W = int(round(small.shape[0] * k)), int(round(small.shape[1] * k))
    src0 = c.resize_u8c3(small, H, W)
    wh, ww = nct.working_size(H, W, 1000)
    full = c.process_pair_fullres(src0, ref, 1000)
    row = {"quality": "24 MP", "images": "demo photographs in0 / tar0" if natural else "committed stand-ins of in0 / tar0", "weights": "synthetic (He-normal, seed 19)",
           "original": [H, W], "working": [wh, ww], "psnr_source_dB": round(psnr(src0, full), 2)}
    row["psnr_fullres2_dB"] = round(psnr(c.process_pair_fullres(src0, ref, 1000, finish=nct.FINISH_UPSAMPLE), full), 2)
    c.set_finish_guided(nct.GuidedParams.default().sigma)
    row["psnr_fullres2_upguide_dB"] = round(psnr(c.process_pair_fullres(src0, ref, 1000, finish=nct.FINISH_UPSAMPLE), full), 2)
    c.set_finish_guided(None)
    work = c.resize_u8c3(src0, wh, ww)
    res = c.process_pair(work, ref)                          # the working-size run: what the fits read
    row["psnr_lut33_dB"] = round(psnr(c.lut_apply(c.pair_fit_lut(33), src0.reshape(-1, 3)).reshape(src0.shape), full), 2)
    emit(row)
    for G in SIZES:
        g = grid_shape(wh, ww, G)
        r = {"quality": "24 MP sweep", "grid": list(g), "psnr_dB": {}}
        for lam in LAMBDAS:
            r["psnr_dB"][str(lam)] = round(psnr(c.grid_apply(c.pair_fit_grid(g, lam), src0), full), 2)
        emit(r)
    S, O = grid_ref.two_gradings()
    for G in SIZES:
        g = (G, G, G if G <= 32 else 32)
        r = {"quality": "two-gradings fixture, mean absolute error", "grid": list(g), "mae": {}}
        for lam in LAMBDAS:
            out = c.grid_apply(c.grid_fit(S, O, g, lam), S)
            r["mae"][str(lam)] = round(float(np.abs(out.astype(np.int64) - O.astype(np.int64)).mean()), 3)
        emit(r)


def main():
    import nct
    import synth
    from caffemodel_io import synthetic_vgg19
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["speed", "quality"])
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

    ws, bs = synthetic_vgg19(19)
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        if "speed" in args.what:
            speed(c, nct, synth, args, emit)
        if "quality" in args.what:
            quality(c, nct, synth, args, emit)


if __name__ == "__main__":
    main()
