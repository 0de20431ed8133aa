"""The guided finish (SPEC §6.10) on the GPU: the seam (host and device-pointer forms, both Lab -> BGR forms) bit for bit against the numpy reference
(tests/finish_guided_ref.py), the clamp, equal sizes, a NaN coefficient, the refusals, the modifier on a pair and on a full-resolution sequence against the composition
of the GPU's own working-size levels and the reference, what the arena holds afterwards, and the CLI's -upguide. All comparisons are equality of bytes / bit patterns."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import finish_guided_ref as gr
import finish_up_ref as fr
import seq_auto_ref as ar
import seq_mc_ref
import synth
from fullres_ref import working_size

pytestmark = pytest.mark.gpu
BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
WH, WW = fr.WORK


def _params(levels=5, flags=0):
    p = nct.Params.default()
    p.levels, p.flags = levels, flags
    return p


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


# ---------------------------------------------------------------- 1-5: the seam
@pytest.mark.parametrize("case,sigma", [(c, gr.SIGMA) for c in range(len(gr.SEAM_CASES))] + [(gr.NONINT, 1.0), (gr.NONINT, 1000.0)])
def test_seam_matches_the_reference(ctx, oracle, case, sigma):
    (h, w), (H, W) = gr.SEAM_CASES[case]
    ab, lab_w, s_full = gr.seam_inputs(oracle, case)
    _, lab = gr.finish_guided(oracle, ab, lab_w, h, w, s_full, sigma)
    for flags, form in ((nct.FLAG_LAB2BGR_CUBE, 1), (0, 0)):
        exp = oracle.lab2bgr(lab, form)
        got = ctx.color_finish_guided(ab, lab_w, h, w, s_full, sigma, _params(flags=flags))
        assert got.shape == (H, W, 3) and np.array_equal(got, exp), (case, form, int((got != exp).sum()))
        assert np.array_equal(ctx.color_finish_guided_dev(ab, lab_w, h, w, s_full, sigma, _params(flags=flags)), exp), (case, form)
    if (H, W) != (h, w) and sigma == gr.SIGMA and min(h, w) > 3:                 # the guide matters: another picture than the bilinear stretch
        assert not np.array_equal(got, ctx.color_finish_upsample(ab, h, w, s_full))


def test_seam_clamps(ctx, oracle):
    ab, lab_w, h, w, s_full = gr.clamp_inputs(oracle)
    exp, lab = gr.finish_guided(oracle, ab, lab_w, h, w, s_full)
    assert (lab == 0).mean() >= 0.01 and (lab == 255).mean() >= 0.01
    assert np.array_equal(ctx.color_finish_guided(ab, lab_w, h, w, s_full), exp)
    assert np.array_equal(ctx.color_finish_guided_dev(ab, lab_w, h, w, s_full), exp)


def test_equal_sizes_are_the_upsampling_finish(ctx, oracle):
    (h, w), _ = gr.SEAM_CASES[0]
    ab, lab_w, s = gr.seam_inputs(oracle, 0)
    exp = ctx.color_finish_upsample(ab, h, w, s)
    for sigma in (1.0, gr.SIGMA):
        assert np.array_equal(ctx.color_finish_guided(ab, lab_w, h, w, s, sigma), exp)
        assert np.array_equal(ctx.color_finish_guided_dev(ab, lab_w, h, w, s, sigma), exp)


def test_a_nan_coefficient_stays_in_its_footprint(ctx, oracle):
    (h, w), (H, W) = gr.SEAM_CASES[gr.NONINT]
    ab, lab_w, s_full = gr.seam_inputs(oracle, gr.NONINT)
    clean = ctx.color_finish_guided(ab, lab_w, h, w, s_full)
    py, px = 15, 12
    bad = ab.copy(); bad[0, py * w + px, 1] = np.nan
    exp, _ = gr.finish_guided(oracle, bad, lab_w, h, w, s_full)
    got = ctx.color_finish_guided(bad, lab_w, h, w, s_full)
    assert np.array_equal(got, exp) and np.array_equal(ctx.color_finish_guided_dev(bad, lab_w, h, w, s_full), exp)
    # the pixels whose taps of non-zero weight include (py, px): offset j = py - s in -1 .. 2 with a non-zero tent
    (sy, fy), (sx, fx) = gr.lin_coef(h, H), gr.lin_coef(w, W)
    iny = np.zeros(H, bool); inx = np.zeros(W, bool)
    for j in (-1, 0, 1, 2):
        iny |= (sy + j == py) & (gr.tent(fy, j) != 0.0)
        inx |= (sx + j == px) & (gr.tent(fx, j) != 0.0)
    foot = iny[:, None] & inx[None, :]
    assert foot.sum() >= 16 and np.array_equal(got[~foot], clean[~foot])
    assert (got[foot] != clean[foot]).any()


def test_seam_refusals(ctx, oracle):
    (h, w), (H, W) = gr.SEAM_CASES[2]
    ab, lab_w, s = gr.seam_inputs(oracle, 2)
    before = ctx.color_finish_guided(ab, lab_w, h, w, s)
    prm, gp = _params(), nct.GuidedParams.default()
    P, G = C.addressof(prm), C.addressof(gp)
    raw = lambda *a: ctx._chk(ctx._l.nct_color_finish_guided_dev(ctx._h, *a))
    d = ctx.dev_alloc(64)

    def refused(call, word):
        with pytest.raises(nct.NctError) as e:
            call()
        assert e.value.code == -2 and word in str(e.value), str(e.value)
    try:
        for args, word in (((None, d, h, w, d, H, W, G, P, d), "null"), ((d, None, h, w, d, H, W, G, P, d), "null"), ((d, d, h, w, None, H, W, G, P, d), "null"),
                           ((d, d, h, w, d, H, W, None, P, d), "null"), ((d, d, h, w, d, H, W, G, None, d), "null"), ((d, d, h, w, d, H, W, G, P, None), "null"),
                           ((d, d, 0, w, d, H, W, G, P, d), "grid"), ((d, d, h, 16385, d, H, 16385, G, P, d), "grid"),
                           ((d, d, h, w, d, h - 1, W, G, P, d), "smaller"), ((d, d, h, w, d, H, w - 1, G, P, d), "smaller"),
                           ((d, d, h, w, d, 16385, W, G, P, d), "target")):
            refused(lambda: raw(*args), word)
        for sigma in (0.0, -1.0, float("nan"), float("inf"), 1e-200, 1e200):
            bad = nct.GuidedParams(sigma)
            refused(lambda: raw(d, d, h, w, d, H, W, C.addressof(bad), P, d), "sigma")
            refused(lambda: ctx.color_finish_guided(ab, lab_w, h, w, s, sigma), "sigma")
            refused(lambda: ctx.set_finish_guided(sigma), "sigma")
    finally:
        ctx.synchronize()
        ctx.dev_free(d)
    out = np.empty_like(s)
    refused(lambda: ctx._chk(ctx._l.nct_color_finish_guided(ctx._h, ab.reshape(-1), lab_w.reshape(-1, 3), h, w, s.reshape(-1, 3)[: (h - 1) * W], h - 1, W, G, P,
                                                             out.reshape(-1, 3))), "smaller")
    assert np.array_equal(ctx.color_finish_guided(ab, lab_w, h, w, s), before)               # the refused calls changed nothing


# ---------------------------------------------------------------- 6: the modifier on a pair
@pytest.mark.parametrize("levels", [5, 1])
def test_pair_with_the_modifier(wctx, oracle, levels):
    src0, ref0 = synth.image(31, 300, 220), synth.image(32, 260, 200)
    prm = _params(levels)
    plain = wctx.process_pair_fullres(src0, ref0, 128, prm, finish=nct.FINISH_UPSAMPLE)
    exact = wctx.process_pair_fullres(src0, ref0, 128, prm)
    small, small_ref = synth.image(41, 120, 96), synth.image(42, 100, 128)
    wctx.set_finish_guided(10.0)
    try:
        got, tm = wctx.process_pair_fullres(src0, ref0, 128, prm, want_timing=True, finish=nct.FINISH_UPSAMPLE)
        assert tm["color_ms"] > 0
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit(src0, got, 9))              # nct_pair_fit_lut works as before
        assert np.array_equal(wctx.process_pair_fullres(src0, ref0, 128, prm), exact)          # the exact finish is not touched
        # a source that needs no shrinking is nct_process_pair
        assert np.array_equal(wctx.process_pair_fullres(small, small_ref, 128, _params(1), finish=nct.FINISH_UPSAMPLE), wctx.process_pair(small, small_ref, _params(1)))
        wctx.set_finish_guided(None)
        assert np.array_equal(wctx.process_pair_fullres(src0, ref0, 128, prm, finish=nct.FINISH_UPSAMPLE), plain)
    finally:
        wctx.set_finish_guided(None)
    assert got.shape == src0.shape and not np.array_equal(got, plain)
    # the GPU's own working-size levels, then the numpy reference on the last level's ab_wls with the shrunk source's Lab image as the guide
    (sh, sw), (rh, rw) = working_size(300, 220, 128), working_size(260, 200, 128)
    S, R = wctx.resize_u8c3(src0, sh, sw), wctx.resize_u8c3(ref0, rh, rw)
    wctx.pair_upload(S, R)
    keep = wctx.pair_run_levels(S.shape, R.shape, prm, want_color=True)
    st = keep["color"][levels - 1]
    lab_w = oracle.bgr2lab(S)
    exp, _ = gr.finish_guided(oracle, st["ab_wls"], lab_w, sh, sw, src0, 10.0, form=0)
    assert np.array_equal(got, exp), int((got != exp).sum())
    assert np.array_equal(got, wctx.color_finish_guided(st["ab_wls"], lab_w, sh, sw, src0, 10.0, prm))


# ---------------------------------------------------------------- 7: the modifier on a full-resolution sequence
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _three_frames(c, frames, auto):
    """a full frame, a propagated frame, an auto frame, then a probe of a fourth (it reads the state and leaves it) -> [(result, maps or decision)], probe"""
    c.seq_set_motion(*MOT)
    outs = [c.seq_frame_levels(frames[0], want_color=False), c.seq_frame_propagate_levels(frames[1]), c.seq_frame_auto(frames[2], auto)]
    return outs, c.seq_probe(frames[3], auto)


def test_sequence_with_the_modifier(wctx, oracle):
    levels = 2
    prm = _params(levels)
    frames, ref0, auto = fr.pan()[:4], synth.image(*fr.REF), nct.seq_auto(*fr.AUTO)
    strip = lambda d: {k: v for k, v in d.items() if k != "probe_ms"}
    # the plain sequence on the shrunk frames: its state, and per frame the coefficients its finish starts from
    S = [wctx.resize_u8c3(f, WH, WW) for f in frames]
    R = wctx.resize_u8c3(ref0, *nct.working_size(*ref0.shape[:2], fr.MAX_SIDE))
    wctx.seq_begin(R, (WH, WW, 3), prm)
    try:
        wctx.seq_set_motion(*MOT)
        pl = [wctx.seq_frame_levels(S[0], want_color=False), wctx.seq_frame_propagate_levels(S[1])]
        dec = wctx.seq_probe(S[2], auto)                                     # what the auto frame will be; then the manual call of that kind, which reports its maps
        pl.append(wctx.seq_frame_propagate_levels(S[2]) if dec["kind"] == ar.PROPAGATED else wctx.seq_frame_levels(S[2], want_color=False))
        plain_probe = wctx.seq_probe(S[3], auto)
    finally:
        wctx.seq_end()
    assert dec["kind"] != ar.SCENE_CUT
    runs = {}
    for on in (False, True):
        wctx.seq_begin_fullres(ref0, frames[0].shape, fr.MAX_SIDE, nct.FINISH_UPSAMPLE, prm)
        try:
            wctx.set_finish_guided(10.0 if on else None)                     # with a sequence open: it takes effect with the next finish
            runs[on] = _three_frames(wctx, frames, auto)
        finally:
            wctx.set_finish_guided(None)
            wctx.seq_end()
    (g_outs, g_probe), (u_outs, u_probe) = runs[True], runs[False]
    # the state is the unguided sequence's and the plain sequence's, word for word
    for t in (0, 1):
        for k in ("ab_blend", "tau_map", "motion"):
            for l in range(levels):
                assert np.array_equal(bits(g_outs[t][1][k][l]), bits(u_outs[t][1][k][l])) and np.array_equal(bits(g_outs[t][1][k][l]), bits(pl[t][1][k][l])), (t, k, l)
    assert strip(g_outs[2][1]) == strip(u_outs[2][1]) == strip(dec) and strip(g_probe) == strip(u_probe) == strip(plain_probe)
    d, hh, ww = [], WH, WW
    for _ in range(5):
        d.insert(0, (hh, ww)); hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    h, w = d[levels - 1]
    for t in range(3):
        _, st = wctx.color_finish(pl[t][1]["ab_blend"][levels - 1], h, w, WH, WW, S[t], prm, want_stages=True)
        exp, _ = gr.finish_guided(oracle, st["ab_wls"], oracle.bgr2lab(S[t]), WH, WW, frames[t], 10.0, form=0)
        assert g_outs[t][0].shape == frames[t].shape and np.array_equal(g_outs[t][0], exp), (t, int((g_outs[t][0] != exp).sum()))
        assert np.array_equal(u_outs[t][0], wctx.color_finish_upsample(st["ab_wls"], WH, WW, frames[t], prm)) and not np.array_equal(g_outs[t][0], u_outs[t][0]), t


# ---------------------------------------------------------------- 8: the arena
def test_arena_holds_no_block_more(weights):
    """the guide is the working-size Lab image the finish already holds: after a guided pair the arena holds exactly what it holds after the unguided upsampling finish"""
    ref0 = synth.image(52, 700, 900)
    held = {}
    src0 = None
    for on in (False, True):
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            if src0 is None:
                src0 = c.resize_u8c3(synth.image(51, 600, 425), 2400, 1700)
        with nct.Context(0) as c:
            c.vgg19_load_raw(*weights)
            if on:
                c.set_finish_guided(10.0)
            out = c.process_pair_fullres(src0, ref0, 1000, _params(1), finish=nct.FINISH_UPSAMPLE)
            assert out.shape == src0.shape
            held[on] = c.counter(nct.CTR_ARENA_BYTES)
    print("arena: guided %d B, unguided %d B" % (held[True], held[False]))
    assert held[True] == held[False]


# ---------------------------------------------------------------- 9: the CLI
def test_cli_upguide(tmp_path, wctx, weights):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    big = synth.image(4, 1100, 700)                                                           # above the driver's working size of 1000: it is shrunk
    Image.fromarray(big[..., ::-1].copy()).save(inp / "big.png")
    small = synth.image(5, 120, 160)
    Image.fromarray(small[..., ::-1].copy()).save(inp / "small.png")
    (inp / "pairs.txt").write_text("big.png small.png 2.0\n")
    prm = _params(1); prm.bds_weight = 2.0; prm.flags = nct.FLAG_LATENCY                      # what the driver runs one pair at a time with
    got = {}
    for name, extra in (("plain", ()), ("guided", ("-upguide", "1")), ("sigma5", ("-upguide", "1", "-upsigma", "5"))):
        out = tmp_path / name
        r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-levels", "1", "-fullres", "2", *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got[name] = np.asarray(Image.open(out / "big_small_2.00.png").convert("RGB"))[..., ::-1]
        assert got[name].shape == big.shape
    # without -upguide the output file is what it was
    assert np.array_equal(got["plain"], wctx.process_pair_fullres(big, small, 1000, prm, finish=nct.FINISH_UPSAMPLE))
    try:
        for name, sigma in (("guided", 10.0), ("sigma5", 5.0)):
            wctx.set_finish_guided(sigma)
            assert np.array_equal(got[name], wctx.process_pair_fullres(big, small, 1000, prm, finish=nct.FINISH_UPSAMPLE)), name
    finally:
        wctx.set_finish_guided(None)
    assert not np.array_equal(got["guided"], got["plain"]) and not np.array_equal(got["guided"], got["sigma5"])
