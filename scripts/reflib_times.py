#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.26 (reference libraries). One JSON line per measurement. Needs a GPU.

    python scripts/reflib_times.py [--reps 20] [--batches 5] [--no-rank]

The match (SPEC §6.21 rule D3: the fill of the column maxima, k_desc_match, k_desc_sums) through nct_descriptor_match_bench and, as the yardstick, k_region_score through
nct_region_score_bench on the same number of multiply-adds: after a warm-up, `reps` launches between two HIP events on the library's stream; median, min and max of
`batches` such means, the two kernels ALTERNATING batch by batch in one process. Cases: a 1936-cell source (700 x 700 at tap 5), C = 512, against 32 entries of 2048
rows — beside it k_region_score on 1936 cells against 65536 seed rows of C = 512 —, and the match at 8 and at 256 entries. Reported beside the time, as ratios only: the
multiply-add rate and its fraction of the int8 matrix-core rate (v_mfma_i32_32x32x32_i8 is 32768 multiply-adds in the 32 cycles of the bf16 form of the same tile: 1024 per
cycle and SIMD, x 4 SIMDs x 256 CUs x 2.4 GHz = 2.5e15 / s), and for the dot2 kernel the fraction of v_dot2c_i32_i16's 79e12 / s. Then one nct_reflib_rank end to end
(forward to the tap, descriptor, match, sums, the waits) beside one nct_process_pair at 700 x 700, synthetic weights, wall clock, median of `batches`.
There is no pass / fail threshold."""
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

I8_MAC_PER_S = 1024 * 4 * 256 * 2.4e9
DOT2_MAC_PER_S = 79e12


def rows8(rng, n, Cc):
    x = rng.standard_normal((n, Cc)).astype(np.float32)
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.rint(x * 127).astype(np.int8)


def rows16(rng, n, Cc):
    x = rng.standard_normal((n, Cc)).astype(np.float32)
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.rint(x * 32767).astype(np.int16)


def stats(ms):
    return {"ms_per_launch": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--no-rank", action="store_true")
    args = ap.parse_args()
    import nct
    rng = np.random.default_rng(1)
    na, Cc, nb = 1936, 512, 2048
    with nct.Context(0) as c:
        print(json.dumps({"device": c.device_name()}), flush=True)
        d_a = c.dev_upload(rows8(rng, na, Cc))
        d_q, d_s, d_o = c.dev_upload(rows16(rng, na, Cc)), c.dev_upload(rows16(rng, 65536, Cc)), c.dev_alloc(na)
        for N in (32, 8, 256):
            offs = (np.arange(N + 1) * nb).astype(np.int32)
            rows = np.tile(rows8(rng, min(N, 32) * nb, Cc), (N // min(N, 32), 1))      # 256 entries: the same 32 eight times (the time does not depend on the values)
            d_r, d_f, d_b = c.dev_upload(rows), c.dev_alloc(8 * N), c.dev_alloc(8 * N)
            mm, ms = [], []
            for _ in range(args.batches):
                mm.append(c.descriptor_match_bench(d_a, na, Cc, d_r, offs, d_f, d_b, args.reps))
                if N == 32:                                      # the yardstick beside it, alternating
                    t = C.c_float(0)
                    c._chk(c._l.nct_region_score_bench(c._h, d_q, na, Cc, d_s, 65536, None, 0, 1024, 700, d_o, args.reps, C.byref(t)))
                    ms.append(t.value)
            macs = na * N * nb * Cc
            r = {"pass": "descriptor_match", "na": na, "C": Cc, "entries": N, "rows_per_entry": nb, **stats(mm), "mac_per_launch": macs,
                 "Tmac_per_s": round(macs / np.median(mm) / 1e9, 1), "fraction_of_i8_mfma_peak": round(macs / np.median(mm) * 1e3 / I8_MAC_PER_S, 4), "reps": args.reps,
                 "batches": args.batches}
            print(json.dumps(r), flush=True)
            if ms:
                macs = na * 65536 * Cc
                print(json.dumps({"pass": "region_score", "cells": na, "C": Cc, "n_in": 65536, "n_out": 0, **stats(ms), "mac_per_launch": macs,
                                  "Tmac_per_s": round(macs / np.median(ms) / 1e9, 1), "fraction_of_dot2_peak": round(macs / np.median(ms) * 1e3 / DOT2_MAC_PER_S, 4),
                                  "match_over_score_speed": round(float(np.median(ms) / np.median(mm)), 2), "reps": args.reps, "batches": args.batches}), flush=True)
            for p in (d_r, d_f, d_b):
                c.dev_free(p)
        for p in (d_a, d_q, d_s, d_o):
            c.dev_free(p)
        if args.no_rank:
            return
        import synth
        from caffemodel_io import synthetic_vgg19
        c.vgg19_load_raw(*synthetic_vgg19(19))
        src, refs = synth.image(1000, 700, 700), [synth.image(1001 + i, 700, 700) for i in range(8)]
        L = nct.RefLib(5)
        for r in refs:
            L.add(c, r)
        c.reflib_rank(L, src); c.process_pair(src, refs[0])     # warm: the library resident, the arena grown
        tr, tp = [], []
        for _ in range(args.batches):
            t0 = time.perf_counter(); c.reflib_rank(L, src); t1 = time.perf_counter(); c.process_pair(src, refs[0]); t2 = time.perf_counter()
            tr.append((t1 - t0) * 1e3); tp.append((t2 - t1) * 1e3)
        print(json.dumps({"pass": "reflib_rank_end_to_end", "side": 700, "tap": 5, "entries": len(refs), "ms": round(float(np.median(tr)), 3), "min_ms": round(min(tr), 3),
                          "max_ms": round(max(tr), 3), "process_pair_ms": round(float(np.median(tp)), 3), "process_pair_min_ms": round(min(tp), 3),
                          "process_pair_max_ms": round(max(tp), 3), "batches": args.batches, "weights": "synthetic"}), flush=True)
        L.close()


if __name__ == "__main__":
    main()
