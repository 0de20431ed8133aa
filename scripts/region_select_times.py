#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.21 (region selection from strokes). One JSON line per measurement. Needs a GPU.

    python scripts/region_select_times.py [--side 700] [--tap 2] [--reps 20] [--batches 5]

The score kernel alone (k_region_score, SPEC §6.16 rule 4) through nct_region_score_bench: after a warm-up launch, `reps` launches between two HIP events on the
library's stream; median, min and max of `batches` such means. Case: a side x side source at `tap` (700 at tap 2: 350 x 350 cells, C = 128) with 4096 + 4096 seeds
and with 64 + 64. The rows are random unit rows as rule 2 makes them. Reported beside the time, as ratios only: the integer-dot rate, cells (n_in + n_out) C / 2
two-element dot instructions per second, and the bytes streamed through the workgroups — per tile of 128 query cells the tile's rows once per seed chunk of 64 and every
seed row once — per second. There is no pass / fail threshold."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))

TAP_C = (64, 128, 256, 512, 512)
TILE_Q, CHUNK_S = 128, 64                   # k_region_select.hip: SC_TQ, SC_TS


def unit_rows(rng, n, Cc):
    x = rng.standard_normal((n, Cc)).astype(np.float32)
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.rint(x * 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=700)
    ap.add_argument("--tap", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    args = ap.parse_args()
    import nct
    rng = np.random.default_rng(1)
    side_t = ((args.side - 1) >> (args.tap - 1)) + 1
    cells, Cc = side_t * side_t, TAP_C[args.tap - 1]
    with nct.Context(0) as c:
        print(json.dumps({"device": c.device_name()}), flush=True)
        d_q, d_o = c.dev_upload(unit_rows(rng, cells, Cc)), c.dev_alloc(cells)
        for n in (4096, 64):
            d_i, d_n = c.dev_upload(unit_rows(rng, n, Cc)), c.dev_upload(unit_rows(rng, n, Cc))
            ms = []
            for _ in range(args.batches):
                t = C.c_float(0)
                c._chk(c._l.nct_region_score_bench(c._h, d_q, cells, Cc, d_i, n, d_n, n, 1024, 700, d_o, args.reps, C.byref(t)))
                ms.append(t.value)
            med = float(np.median(ms))
            dots = cells * 2 * n * Cc / 2
            tiles, chunks = -(-cells // TILE_Q), -(-2 * n // CHUNK_S)
            streamed = tiles * (chunks * TILE_Q + 2 * n) * Cc * 2
            print(json.dumps({"pass": "region_score", "cells": cells, "C": Cc, "n_in": n, "n_out": n, "ms_per_launch": round(med, 4), "min_ms": round(min(ms), 4),
                              "max_ms": round(max(ms), 4), "dot2_per_launch": dots, "Tdot2_per_s": round(dots / med / 1e9, 2), "bytes_streamed": streamed,
                              "streamed_GBps": round(streamed / med / 1e6, 1), "reps": args.reps, "batches": args.batches}), flush=True)
            c.dev_free(d_i); c.dev_free(d_n)
        c.dev_free(d_q); c.dev_free(d_o)


if __name__ == "__main__":
    main()
