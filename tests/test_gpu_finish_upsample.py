"""The upsampling finish (SPEC §6.8) on the GPU: the seam (host and device-pointer forms) bit for bit against the oracle's chain, the clamp, the whole pair against
the oracle composition and against the GPU's own levels + seam, the identities, the refusals, what the arena holds afterwards, and the CLI's -fullres 2."""
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import synth
from finish_up_ref import oracle_finish_upsample, SEAM_CASES, seam_inputs, clamp_inputs
from fullres_ref import oracle_finish, working_size

pytestmark = pytest.mark.gpu
BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


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


@pytest.mark.parametrize("case", range(len(SEAM_CASES)))
def test_seam_matches_the_oracle_chain(ctx, oracle, case):
    (h, w), (H, W) = SEAM_CASES[case]
    ab, s_full = seam_inputs(case)
    _, lab = oracle_finish_upsample(oracle, ab, h, w, s_full)
    for flags, form in ((nct.FLAG_LAB2BGR_CUBE, 1), (0, 0)):
        exp = oracle.lab2bgr(lab, form)
        got = ctx.color_finish_upsample(ab, h, w, s_full, _params(flags=flags))
        assert got.shape == (H, W, 3) and np.array_equal(got, exp), (case, form, int((got != exp).sum()))
        assert np.array_equal(ctx.color_finish_upsample_dev(ab, h, w, s_full, _params(flags=flags)), exp), (case, form)


def test_seam_clamps(ctx, oracle):
    ab, h, w, s_full = clamp_inputs()
    exp, lab = oracle_finish_upsample(oracle, ab, h, w, s_full)
    assert (lab == 0).mean() >= 0.01 and (lab == 255).mean() >= 0.01
    assert np.array_equal(ctx.color_finish_upsample(ab, h, w, s_full), exp)
    assert np.array_equal(ctx.color_finish_upsample_dev(ab, h, w, s_full), exp)


def test_seam_equals_the_gpu_chain(ctx):
    """equal sizes, through the library's own exact finish: U1 is a copy there, so the upsampling finish of the exact finish's ab_wls is the exact finish's bytes"""
    h, w = 61, 47
    ab, s = seam_inputs(0)
    exp, st = ctx.color_finish(ab, h, w, h, w, s, want_stages=True)
    assert np.array_equal(ctx.color_finish_upsample(st["ab_wls"], h, w, s), exp)


def test_seam_refusals(ctx):
    ab, s = seam_inputs(1)
    (h, w), (H, W) = SEAM_CASES[1]
    prm = _params()
    out = np.empty_like(s)
    import ctypes as C
    raw = lambda *a: ctx._chk(ctx._l.nct_color_finish_upsample_dev(ctx._h, *a))
    d = ctx.dev_alloc(64)
    try:
        for args, word in (((None, h, w, d, H, W, C.addressof(prm), d), "null"), ((d, h, w, None, H, W, C.addressof(prm), d), "null"),
                           ((d, h, w, d, H, W, C.addressof(prm), None), "null"), ((d, h, w, d, H, W, None, d), "null"),
                           ((d, 0, w, d, H, W, C.addressof(prm), d), "grid"), ((d, h, 16385, d, H, 16385, C.addressof(prm), d), "grid"),
                           ((d, h, w, d, h - 1, W, C.addressof(prm), d), "smaller"), ((d, h, w, d, H, w - 1, C.addressof(prm), d), "smaller"),
                           ((d, h, w, d, 16385, W, C.addressof(prm), d), "target")):
            with pytest.raises(nct.NctError) as e:
                raw(*args)
            assert e.value.code == -2 and word in str(e.value), (args[1:3], str(e.value))
    finally:
        ctx.synchronize()
        ctx.dev_free(d)
    with pytest.raises(nct.NctError) as e:
        ctx._chk(ctx._l.nct_color_finish_upsample(ctx._h, ab.reshape(-1), h, w, s.reshape(-1, 3)[: (h - 1) * W], h - 1, W, C.addressof(prm), out.reshape(-1, 3)))
    assert e.value.code == -2 and "smaller" in str(e.value)


def _oracle_pair_upsample(oracle, src0, ref0, max_side, ws, bs, levels):
    """SPEC §6.8 composed from the oracle (mirrors test_gpu_fullres._oracle_pair_fullres): shrink, the pair at working size, the last level's S1 from its guide /
    error / labels / kNN graph, its working-size finish's ab_wls, then the chain on src0"""
    (sh, sw), (rh, rw) = working_size(*src0.shape[:2], max_side), working_size(*ref0.shape[:2], max_side)
    S, R = oracle.resize_u8c3(src0, sh, sw), oracle.resize_u8c3(ref0, rh, rw)
    _, keep = oracle.process_pair(S, R, ws, bs, params={"levels": levels}, want_nnf=True)
    l = levels - 1
    feat5 = oracle.vgg19_features(S, ws, bs)[4]
    labels, nl = oracle.cluster_features(feat5, 10, 11, 1)
    simg = [S]
    for _ in range(4):
        h, w = simg[0].shape[:2]
        simg.insert(0, oracle.resize_u8c3(simg[0], (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    s_l = simg[l]
    knn_id, knn_w = oracle.knn_graph(oracle.bgr2lab(s_l), labels, nl, 1 << l)
    _, stages = oracle.local_color_transfer(keep["err"][l], s_l, keep["guide"][l], S, knn_id, knn_w, l, want_stages=True)
    h, w = s_l.shape[:2]
    _, st = oracle_finish(oracle, stages["ab_nonlocal"], h, w, sh, sw, S)
    return oracle_finish_upsample(oracle, st["ab_wls"], sh, sw, src0)[0]


@pytest.mark.parametrize("levels", [5, 1])
def test_pair_matches_the_oracle_and_its_own_seam(wctx, oracle, weights, levels):
    src0, ref0 = synth.image(31, 300, 220), synth.image(32, 260, 200)
    prm = _params(levels)
    got, tm = wctx.process_pair_fullres(src0, ref0, 128, prm, want_timing=True, finish=nct.FINISH_UPSAMPLE)
    assert got.shape == src0.shape
    exp = _oracle_pair_upsample(oracle, src0, ref0, 128, *weights, levels)
    assert np.array_equal(got, exp), int(np.abs(got.astype(int) - exp.astype(int)).max())
    # the GPU's own levels, then the seam; the timing's WLS is the working-size solve
    (sh, sw), (rh, rw) = working_size(300, 220, 128), working_size(260, 200, 128)
    S, R = wctx.resize_u8c3(src0, sh, sw), wctx.resize_u8c3(ref0, rh, rw)
    wctx.pair_upload(S, R)
    keep = wctx.pair_run_levels(S.shape, R.shape, prm, want_color=True)
    st = keep["color"][levels - 1]
    assert np.array_equal(got, wctx.color_finish_upsample(st["ab_wls"], sh, sw, src0, prm))
    assert tm["wls_iters"][levels - 1] == max(st["wls_iters"]) and tm["color_ms"] > 0
    # another picture than the exact finish, and the exact finish is nct_process_pair_fullres
    exact = wctx.process_pair_fullres(src0, ref0, 128, prm)
    assert not np.array_equal(got, exact)
    from ctypes import addressof
    out = np.empty_like(src0)
    wctx._chk(wctx._l.nct_process_pair_fullres_finish(wctx._h, src0.reshape(-1, 3), 300, 220, ref0.reshape(-1, 3), 260, 200, 128, nct.FINISH_EXACT, addressof(prm),
                                                      out.reshape(-1, 3), None))
    assert np.array_equal(out, exact)


def test_identity_and_refusals(wctx):
    src0, ref0, big_ref = synth.image(41, 120, 96), synth.image(42, 100, 128), synth.image(43, 300, 200)
    prm = _params(1)
    plain = wctx.process_pair(src0, ref0, prm)
    assert np.array_equal(wctx.process_pair_fullres(src0, ref0, 128, prm, finish=nct.FINISH_UPSAMPLE), plain)
    R = wctx.resize_u8c3(big_ref, *working_size(300, 200, 128))
    assert np.array_equal(wctx.process_pair_fullres(src0, big_ref, 128, prm, finish=nct.FINISH_UPSAMPLE), wctx.process_pair(src0, R, prm))
    for bad in (7, -1, 2):
        with pytest.raises(nct.NctError) as e:
            wctx.process_pair_fullres(src0, ref0, 128, prm, finish=bad)
        assert e.value.code == -2 and "finish" in str(e.value)
    assert np.array_equal(wctx.process_pair(src0, ref0, prm), plain)                            # a refused call changed nothing


def test_pair_fit_lut_reads_the_full_result(wctx):
    src0, ref0 = synth.image(31, 300, 220), synth.image(32, 260, 200)
    out = wctx.process_pair_fullres(src0, ref0, 128, _params(1), finish=nct.FINISH_UPSAMPLE)
    assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit(src0, out, 9))


def test_arena_holds_two_images_more(weights):
    """after the upsampling finish on a 2400 x 1700 source the arena may exceed what nct_process_pair on the shrunk pair leaves by at most 16 B per original pixel
    (two 3-byte images plus the rounding of the arena's blocks); the exact finish needs more than 48 B per pixel (test_gpu_fullres.test_scale_and_limits)"""
    src0 = None
    ref0 = synth.image(52, 700, 900)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        src0 = c.resize_u8c3(synth.image(51, 600, 425), 2400, 1700)
        out = c.process_pair_fullres(src0, ref0, 1000, _params(5), finish=nct.FINISH_UPSAMPLE)
        assert out.shape == src0.shape and np.abs(out.astype(int) - src0.astype(int)).mean() > 1.0
        up = c.counter(nct.CTR_ARENA_BYTES)
    (sh, sw), (rh, rw) = working_size(2400, 1700, 1000), working_size(700, 900, 1000)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        S, R = c.resize_u8c3(src0, sh, sw), c.resize_u8c3(ref0, rh, rw)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        c.process_pair(S, R, _params(5))
        plain = c.counter(nct.CTR_ARENA_BYTES)
    print("arena: upsampling finish %d B, working-size pair %d B, difference %.2f B per original pixel" % (up, plain, (up - plain) / (2400 * 1700)))
    assert up - plain <= 16 * 2400 * 1700


def test_cli_fullres_2(tmp_path, wctx, weights):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    big = synth.image(4, 1100, 700)
    Image.fromarray(big[..., ::-1].copy()).save(inp / "big.jpg", quality=90, subsampling=2)
    small = synth.image(5, 120, 160)
    Image.fromarray(small[..., ::-1].copy()).save(inp / "small.png")
    (inp / "pairs.txt").write_text("big.jpg small.png 2.0\n")
    dec = np.asarray(Image.open(inp / "big.jpg").convert("RGB"))[..., ::-1]
    out = tmp_path / "out"
    r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-levels", "1", "-fullres", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.asarray(Image.open(out / "big_small_2.00.png").convert("RGB"))[..., ::-1]
    prm = _params(1); prm.bds_weight = 2.0
    assert got.shape == (1100, 700, 3)
    assert np.array_equal(got, wctx.process_pair_fullres(dec, small, 1000, prm, finish=nct.FINISH_UPSAMPLE))
