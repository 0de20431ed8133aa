#!/usr/bin/env python3
"""The sweep behind the default lambda of the look-up table fit. CPU only: the results come from the oracle (the CPU form of nct_process_pair,
synthetic VGG19), the fit and the apply from the numpy reference tests/lut_ref.py. Per pair the table is fitted on the even pixels and apply(S) is compared with O on
the odd pixels; prints one JSON line per (pair, N) with the PSNR per lambda and the mean rows at the end.

    python scripts/lut_lambda_sweep.py [--sizes 17,33] [--standins in0,in2,in4]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))
LAMBDAS = (0.1, 0.3, 1.0, 3.0, 10.0)


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def main():
    import lut_ref
    import natural_inputs
    import oracle_bind
    import synth
    from caffemodel_io import synthetic_vgg19
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="17,33")
    ap.add_argument("--standins", default="in0,in2,in4")
    args = ap.parse_args()
    orc = oracle_bind.load()
    ws, bs = synthetic_vgg19(19)
    pairs = {"synthetic 56x64": (synth.image(1000, 56, 64), synth.image(1001, 48, 64)), "synthetic 120x100": (synth.image(7, 120, 100), synth.image(8, 90, 110))}
    d = natural_inputs.require()
    load = lambda n: np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, n + ".png")).convert("RGB"))[..., ::-1])
    for n in [t for t in args.standins.split(",") if t]:
        pairs["stand-in " + n] = (load(n), load(n.replace("in", "tar")))
    rows = []
    for name, (src, ref) in pairs.items():
        res = orc.process_pair(src, ref, ws, bs)
        s, o = src.reshape(-1, 3), res.reshape(-1, 3)
        for N in [int(t) for t in args.sizes.split(",")]:
            W, R = lut_ref.splat(s[0::2], o[0::2], N)
            row = {"pair": name, "N": N, "natural": name.startswith("stand-in"), "psnr": {}}
            for lam in LAMBDAS:
                lut = lut_ref.table(lut_ref.solve(W, R, N, lam), N)
                row["psnr"][str(lam)] = round(psnr(lut_ref.apply(lut, N, s[1::2]), o[1::2]), 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    for kind in (False, True):
        sel = [r for r in rows if r["natural"] == kind]
        if sel:
            print(json.dumps({"mean": "natural stand-ins" if kind else "synthetic", "psnr": {str(l): round(float(np.mean([r["psnr"][str(l)] for r in sel])), 3) for l in LAMBDAS}}))


if __name__ == "__main__":
    main()
