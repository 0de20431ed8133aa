#!/usr/bin/env python3
"""The numbers of DESIGN.md §3.14 (the upsampling finish and full-resolution sequences) and §3.15 (the guided finish). One JSON line per measurement. Needs a GPU.

    python scripts/finish_up_times.py kernels --mp 24      one source size (2, 8 or 24 MP, working size 666 x 1000): nct_color_finish_upsample_dev, wall time of
                                                           `reps` enqueued calls between two synchronisations, and the exact finish twice (its bgr2lab, resize_f64c3 x2,
                                                           apply and lab2bgr launches at the original size are the chain the new kernel replaces). Per-kernel times:
                                                           run it under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python scripts/finish_up_times.py kernels --mp 24`
    python scripts/finish_up_times.py report DIR/k_kernel_stats.csv --mp 24
                                                           the chain's kernels summed (average per launch, resize counted twice) beside k_finish_up, GB/s on 6 B/px
    python scripts/finish_up_times.py frames               1920 x 1080 and 3840 x 2160 clips, max_side 1000, motion on: host wall time of a full and of a propagated frame
                                                           (median of five after a warm-up of each kind) for the exact finish, the upsampling finish and the working-size
                                                           sequence on the shrunk frames; WLS iterations of the last level and the arena
    python scripts/finish_up_times.py quality              the nine stand-in pairs, content image upscaled to a longer side of 2000: PSNR of the upsampling finish and of the
                                                           table of the working-size pair (-lut 33 -lutfull 1) against the exact finish; one five-frame pan: transform flicker
    python scripts/finish_up_times.py guided-kernels --mp 24
                                                           nct_color_finish_upsample_dev and nct_color_finish_guided_dev (sigma 10) on the same maps and source, wall time of
                                                           `reps` enqueued calls each; under rocprofv3 as above the stats hold k_finish_up and k_finish_guided side by side
    python scripts/finish_up_times.py guided-report DIR/k_kernel_stats.csv --mp 24
                                                           the two kernels' average times, their ratio, Gpx/s
    python scripts/finish_up_times.py guided-quality       the nine stand-in pairs as in `quality`: PSNR against the exact finish of the bilinear upsampling finish and of the
                                                           guided one at sigma 5, 10 and 20
    python scripts/finish_up_times.py guided-frames --mp 24
                                                           one pair at that source size (max_side 1000): host wall time and color_ms (the colour stage, WLS included) of the upsampling finish, the guided one
                                                           and the exact finish (median of three after a warm-up)
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "neural-color-transfer_amd", "python"))

SIZES = {2: (1155, 1732), 8: (2309, 3464), 24: (4000, 6000)}
CHAIN = (("k_bgr2lab", 1), ("k_resize_f64c3", 2), ("k_apply", 1), ("k_lab2bgr", 1))


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def kernels(args):
    import nct
    import synth
    from fullres_ref import smooth_ab
    H, W = SIZES[args.mp]
    h, w = nct.working_size(H, W, 1000)
    ab = smooth_ab(7, h, w)
    with nct.Context(0) as c:
        src = c.resize_u8c3(synth.image(61, 600, 400), H, W)
        prm = nct.Params.default()
        import ctypes as C
        d_ab, d_s, d_o = c.dev_upload(ab.reshape(-1)), c.dev_upload(src), c.dev_alloc(3 * H * W)
        call = lambda: c._chk(c._l.nct_color_finish_upsample_dev(c._h, d_ab, h, w, d_s, H, W, C.addressof(prm), d_o))
        call(); c.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        c.synchronize()
        us = (time.perf_counter() - t0) / args.reps * 1e6
        print(json.dumps({"call": "color_finish_upsample_dev", "mp": args.mp, "H": H, "W": W, "h": h, "w": w, "us_per_call": round(us, 1), "reps": args.reps,
                          "GBps_on_6B_per_px": round(6 * H * W / us / 1e3, 1)}), flush=True)
        up = c.dev_download(d_o, (H, W, 3), np.uint8)
        for p in (d_ab, d_s, d_o):
            c.dev_free(p)
        # the chain's kernels at the original size run inside the exact finish (with an S2 solve between them, which the report leaves out)
        for _ in range(2):
            t0 = time.perf_counter()
            exact = c.color_finish(ab, h, w, h, w, src, prm)
            ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"call": "color_finish (exact, host pointers)", "mp": args.mp, "ms": round(ms, 1), "psnr_upsample_vs_exact_of_the_same_maps": round(psnr(up, exact), 2)}), flush=True)


def report(args):
    H, W = SIZES[args.mp]
    rows = {r["Name"]: r for r in csv.DictReader(open(args.csv))}
    avg = lambda pat: [float(r["AverageNs"]) / 1e3 for n, r in rows.items() if re.search(r"\b" + pat + r"\b", n)]
    chain = {}
    for name, times in CHAIN:
        a = avg(name)
        chain[name] = round(sum(a) / max(len(a), 1) * times, 1)
    fu = avg("k_finish_up")
    fu = sum(fu) / max(len(fu), 1)
    total = sum(chain.values())
    print(json.dumps({"mp": args.mp, "chain_us": chain, "chain_total_us": round(total, 1), "k_finish_up_us": round(fu, 1), "speedup": round(total / fu, 2) if fu else None,
                      "k_finish_up_GBps_on_6B_per_px": round(6 * H * W / fu / 1e3, 1) if fu else None}))


def guided_kernels(args):
    import ctypes as C
    import nct
    import synth
    from fullres_ref import smooth_ab
    H, W = SIZES[args.mp]
    h, w = nct.working_size(H, W, 1000)
    ab = smooth_ab(7, h, w)
    with nct.Context(0) as c:
        src = c.resize_u8c3(synth.image(61, 600, 400), H, W)
        lab_w = c.bgr2lab(c.resize_u8c3(src, h, w))
        prm, gp = nct.Params.default(), nct.GuidedParams.default()
        d_ab, d_lw, d_s, d_o = c.dev_upload(ab.reshape(-1)), c.dev_upload(lab_w), c.dev_upload(src), c.dev_alloc(3 * H * W)
        calls = {"color_finish_upsample_dev": lambda: c._chk(c._l.nct_color_finish_upsample_dev(c._h, d_ab, h, w, d_s, H, W, C.addressof(prm), d_o)),
                 "color_finish_guided_dev": lambda: c._chk(c._l.nct_color_finish_guided_dev(c._h, d_ab, d_lw, h, w, d_s, H, W, C.addressof(gp), C.addressof(prm), d_o))}
        for name, call in calls.items():
            call(); c.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call()
            c.synchronize()
            us = (time.perf_counter() - t0) / args.reps * 1e6
            print(json.dumps({"call": name, "mp": args.mp, "H": H, "W": W, "h": h, "w": w, "us_per_call": round(us, 1), "reps": args.reps,
                              "Gpx_per_s": round(H * W / us / 1e3, 2)}), flush=True)
        for p in (d_ab, d_lw, d_s, d_o):
            c.dev_free(p)


def guided_report(args):
    H, W = SIZES[args.mp]
    rows = {r["Name"]: r for r in csv.DictReader(open(args.csv))}
    avg = lambda pat: [float(r["AverageNs"]) / 1e3 for n, r in rows.items() if re.search(r"\b" + pat + r"\b", n)]
    fu, fg = avg("k_finish_up"), avg("k_finish_guided")
    fu, fg = sum(fu) / max(len(fu), 1), sum(fg) / max(len(fg), 1)
    print(json.dumps({"mp": args.mp, "k_finish_up_us": round(fu, 1), "k_finish_guided_us": round(fg, 1), "guided_over_bilinear": round(fg / fu, 2) if fu else None,
                      "k_finish_guided_Gpx_per_s": round(H * W / fg / 1e3, 2) if fg else None}))


def guided_quality(args):
    import nct
    import natural_inputs
    from PIL import Image
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    d = natural_inputs.require()
    ld = lambda n: np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, n + ".png")).convert("RGB"))[..., ::-1])
    cases = [("in0", "tar0", 2.0), ("in1", "tar1", 2.0), ("in2", "tar2", 2.0), ("in3", "tar3", 2.0)] + [("in4", "tar4", b) for b in (0.0, 1.0, 2.0, 4.0, 8.0)]
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        for s, r, bds in cases:
            src, ref = ld(s), ld(r)
            k = 2000.0 / max(src.shape[:2])
            src0 = c.resize_u8c3(src, int(round(src.shape[0] * k)), int(round(src.shape[1] * k)))
            prm = nct.Params.default(); prm.bds_weight = bds
            exact = c.process_pair_fullres(src0, ref, 1000, prm)
            row = {"pair": "%s/%s bds %g" % (s, r, bds), "source": "%dx%d" % src0.shape[1::-1],
                   "psnr_bilinear_vs_exact": round(psnr(c.process_pair_fullres(src0, ref, 1000, prm, finish=nct.FINISH_UPSAMPLE), exact), 2)}
            for sigma in (5.0, 10.0, 20.0):
                c.set_finish_guided(sigma)
                row["psnr_guided_sigma_%g_vs_exact" % sigma] = round(psnr(c.process_pair_fullres(src0, ref, 1000, prm, finish=nct.FINISH_UPSAMPLE), exact), 2)
                c.set_finish_guided(None)
            print(json.dumps(row), flush=True)


def guided_frames(args):
    import nct
    import synth
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    H, W = SIZES[args.mp]
    ref = synth.image(62, 800, 640)
    prm = nct.Params.default()
    prm.flags = nct.FLAG_LATENCY
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        src0 = c.resize_u8c3(synth.image(61, 600, 400), H, W)
        for mode, finish, sigma in (("upsample", nct.FINISH_UPSAMPLE, None), ("guided", nct.FINISH_UPSAMPLE, 10.0), ("exact", nct.FINISH_EXACT, None)):
            c.set_finish_guided(sigma)
            ms, color = [], []
            for t in range(4):
                t0 = time.perf_counter()
                _, tm = c.process_pair_fullres(src0, ref, 1000, prm, want_timing=True, finish=finish)
                if t:
                    ms.append((time.perf_counter() - t0) * 1e3); color.append(tm["color_ms"])
            c.set_finish_guided(None)
            print(json.dumps({"pair": "%dx%d" % (W, H), "mode": mode, "host_ms_median": round(float(np.median(ms)), 1), "host_ms_range": [round(min(ms), 1), round(max(ms), 1)],
                              "color_ms_median": round(float(np.median(color)), 1), "wls_ms_last": round(tm["wls_ms"], 1)}), flush=True)


def clip(c, H, W, n, step):
    """n frames of a window that moves `step` px per frame over an upscaled synth image, with fresh noise per frame"""
    import synth
    rng = np.random.default_rng(5)
    base = c.resize_u8c3(synth.image(1000, H // 4, (W + step * (n - 1)) // 4 + 1), H, W + step * (n - 1))
    return [np.clip(np.rint(base[:, step * t:step * t + W].astype(np.float32) + rng.normal(0.0, 2.0, (H, W, 3)).astype(np.float32)), 0, 255).astype(np.uint8) for t in range(n)]


def frames(args):
    import nct
    import synth
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    ref = synth.image(62, 800, 640)
    prm = nct.Params.default()
    prm.flags = nct.FLAG_LATENCY                      # one sequence in flight
    for (H, W) in ((1080, 1920), (2160, 3840)):
        with nct.Context(0) as c:
            clip0 = clip(c, H, W, 12, 16)
        for mode in ("working", "exact", "upsample"):
            with nct.Context(0) as c:                 # its own arena per row
                c.vgg19_load_raw(ws, bs)
                fs = clip0
                wh, ww = nct.working_size(H, W, 1000)
                if mode == "working":
                    fs = [c.resize_u8c3(f, wh, ww) for f in fs]
                    c.seq_begin(ref, fs[0].shape, prm)
                else:
                    c.seq_begin_fullres(ref, fs[0].shape, 1000, nct.FINISH_EXACT if mode == "exact" else nct.FINISH_UPSAMPLE, prm)
                c.seq_set_motion()
                c.seq_frame(fs[0]); c.seq_frame_propagate(fs[1])
                full, prop, it_full, it_prop = [], [], [], []
                for t in range(2, 12):
                    t0 = time.perf_counter()
                    _, tm = (c.seq_frame if t % 2 == 0 else c.seq_frame_propagate)(fs[t], want_timing=True)
                    ms = (time.perf_counter() - t0) * 1e3
                    (full if t % 2 == 0 else prop).append(ms)
                    (it_full if t % 2 == 0 else it_prop).append(tm["wls_iters"][4])
                arena = c.counter(nct.CTR_ARENA_BYTES)
                c.seq_end()
            print(json.dumps({"frames": "%dx%d" % (W, H), "working": "%dx%d" % (ww, wh), "mode": mode, "full_ms_median": round(float(np.median(full)), 1),
                              "full_ms_range": [round(min(full), 1), round(max(full), 1)], "prop_ms_median": round(float(np.median(prop)), 1),
                              "prop_ms_range": [round(min(prop), 1), round(max(prop), 1)], "wls_iters_full": it_full, "wls_iters_prop": it_prop,
                              "arena_GB": round(arena / 1e9, 2)}), flush=True)


def quality(args):
    import nct
    import natural_inputs
    import seq_ref
    from PIL import Image
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    d = natural_inputs.require()
    ld = lambda n: np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, n + ".png")).convert("RGB"))[..., ::-1])
    cases = [("in0", "tar0", 2.0), ("in1", "tar1", 2.0), ("in2", "tar2", 2.0), ("in3", "tar3", 2.0)] + [("in4", "tar4", b) for b in (0.0, 1.0, 2.0, 4.0, 8.0)]
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        for s, r, bds in cases:
            src, ref = ld(s), ld(r)
            k = 2000.0 / max(src.shape[:2])
            src0 = c.resize_u8c3(src, int(round(src.shape[0] * k)), int(round(src.shape[1] * k)))
            prm = nct.Params.default(); prm.bds_weight = bds
            exact = c.process_pair_fullres(src0, ref, 1000, prm)
            up = c.process_pair_fullres(src0, ref, 1000, prm, finish=nct.FINISH_UPSAMPLE)
            wh, ww = nct.working_size(*src0.shape[:2], 1000)
            S = c.resize_u8c3(src0, wh, ww)
            R = c.resize_u8c3(ref, *nct.working_size(*ref.shape[:2], 1000))
            work = c.process_pair(S, R, prm)
            lut = c.lut_apply(c.pair_fit_lut(33), src0)
            scaled = c.resize_u8c3(work, *src0.shape[:2])
            print(json.dumps({"pair": "%s/%s bds %g" % (s, r, bds), "source": "%dx%d" % src0.shape[1::-1], "ratio": round(src0.shape[1] / ww, 2),
                              "psnr_upsample_vs_exact": round(psnr(up, exact), 2), "psnr_lut33_vs_exact": round(psnr(lut, exact), 2),
                              "psnr_upscaled_working_result_vs_exact": round(psnr(scaled, exact), 2)}), flush=True)
        # one five-frame pan over in0 upscaled: a 1500 x 2000 window moving 16 px per frame
        base = ld("in0")
        k = 2064.0 / base.shape[1]
        base = c.resize_u8c3(base, max(int(round(base.shape[0] * k)), 1500), 2064)
        rng = np.random.default_rng(5)
        fs = [seq_ref._noisy(base[:1500, 16 * t:16 * t + 2000], rng, 2.0) for t in range(5)]
        ref = ld("tar0")
        prm = nct.Params.default()
        wh, ww = nct.working_size(1500, 2000, 1000)
        row = {"pan": "5 frames of 2000x1500, 16 px per frame, every frame full, motion on"}
        for mode in ("exact", "upsample", "working"):
            src = fs if mode != "working" else [c.resize_u8c3(f, wh, ww) for f in fs]
            if mode == "working":
                c.seq_begin(c.resize_u8c3(ref, *nct.working_size(*ref.shape[:2], 1000)), src[0].shape, prm)
            else:
                c.seq_begin_fullres(ref, src[0].shape, 1000, nct.FINISH_EXACT if mode == "exact" else nct.FINISH_UPSAMPLE, prm)
            c.seq_set_motion()
            outs = [c.seq_frame(f) for f in src]
            c.seq_end()
            row["transform_flicker_" + mode] = round(seq_ref.transform_flicker(outs, src), 4)
            pairs = [c.process_pair_fullres(f, ref, 1000, prm, finish=nct.FINISH_UPSAMPLE if mode == "upsample" else 0) if mode != "working"
                     else c.process_pair(f, c.resize_u8c3(ref, *nct.working_size(*ref.shape[:2], 1000)), prm) for f in src]
            row["transform_flicker_" + mode + "_independent_pairs"] = round(seq_ref.transform_flicker(pairs, src), 4)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernels", "report", "frames", "quality", "guided-kernels", "guided-report", "guided-quality", "guided-frames"))
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--mp", type=int, default=24, choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    {"kernels": kernels, "report": report, "frames": frames, "quality": quality, "guided-kernels": guided_kernels, "guided-report": guided_report,
     "guided-quality": guided_quality, "guided-frames": guided_frames}[args.what](args)


if __name__ == "__main__":
    main()
