"""Full-resolution output (SPEC §6.1) on the GPU: the finish seam (nct_color_finish) and the whole pair (nct_process_pair_fullres) bit for bit against the
oracle's stages, the identity rule, the pipeline against its own seam at ~4 MP, scale and limits, and the CLI's -fullres flag."""
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import synth
from fullres_ref import oracle_finish, smooth_ab, s2_levels, working_size

pytestmark = pytest.mark.gpu
BIN = os.path.join(nct.PKG_ROOT, "bin", "neural_color_transfer")


def _params(levels=5, flags=0):
    p = nct.Params.default()
    p.levels, p.flags = levels, flags
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# (level grid h x w, working size, target H x W): equal size (the x4 branch), 2x, a non-integer ratio, a side above 4096, a 10-level S2 hierarchy
SEAM_CASES = [((61, 47), (61, 47), (61, 47)),
              ((61, 47), (61, 47), (122, 94)),
              ((31, 24), (61, 47), (250, 171)),
              ((210, 16), (210, 16), (4200, 320)),
              ((375, 375), (375, 375), (3000, 3000))]


@pytest.mark.parametrize("case", range(len(SEAM_CASES)))
def test_color_finish_matches_the_oracle(ctx, oracle, case):
    (h, w), (wh, ww), (H, W) = SEAM_CASES[case]
    if case == 4:
        assert s2_levels(H, W) >= 10
    ab = smooth_ab(100 + case, h, w)
    s_full = synth.image(200 + case, H, W)
    _, exp = oracle_finish(oracle, ab, h, w, wh, ww, s_full)
    for flags, form in ((nct.FLAG_LAB2BGR_CUBE, 1), (nct.FLAG_LATENCY, 0)):
        got, st = ctx.color_finish(ab, h, w, wh, ww, s_full, _params(flags=flags), want_stages=True)
        assert np.array_equal(got, oracle.lab2bgr(exp["lab"], form)), (case, flags)
        for k in ("ab_up", "roughness", "ab_wls"):
            assert np.array_equal(_bits(st[k]), _bits(exp[k])), (case, flags, k)
        assert list(st["wls_iters"]) == list(exp["wls_iters"]), (case, flags)


def _oracle_pair_fullres(oracle, src0, ref0, max_side, ws, bs, levels):
    """SPEC §6.1 composed from the oracle: shrink, the pair at working size, the last level's S1 from its guide / error / labels / kNN graph, the finish on src0"""
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
    out, _ = oracle_finish(oracle, stages["ab_nonlocal"], h, w, sh, sw, src0)
    return out


@pytest.mark.parametrize("levels", [5, 1])
def test_pair_fullres_matches_the_oracle(ctx, oracle, levels):
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    ctx.vgg19_load_raw(ws, bs)
    src0, ref0 = synth.image(31, 300, 220), synth.image(32, 260, 200)
    got = ctx.process_pair_fullres(src0, ref0, 128, _params(levels))
    assert got.shape == src0.shape
    exp = _oracle_pair_fullres(oracle, src0, ref0, 128, ws, bs, levels)
    assert np.array_equal(got, exp), int(np.abs(got.astype(int) - exp.astype(int)).max())


@pytest.mark.parametrize("levels", [1, 5])
def test_identity_when_nothing_or_only_the_reference_shrinks(ctx, levels):
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    ctx.vgg19_load_raw(ws, bs)
    src0, ref0, big_ref = synth.image(41, 120, 96), synth.image(42, 100, 128), synth.image(43, 300, 200)
    prm = _params(levels)
    assert np.array_equal(ctx.process_pair_fullres(src0, ref0, 128, prm), ctx.process_pair(src0, ref0, prm))
    R = ctx.resize_u8c3(big_ref, *working_size(300, 200, 128))
    assert np.array_equal(ctx.process_pair_fullres(src0, big_ref, 128, prm), ctx.process_pair(src0, R, prm))


def test_pipeline_equals_its_seam_at_4mp(ctx):
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    ctx.vgg19_load_raw(ws, bs)
    src0 = ctx.resize_u8c3(synth.image(51, 600, 425), 2400, 1700)
    ref0 = synth.image(52, 700, 900)
    prm = _params(5)
    got, tm = ctx.process_pair_fullres(src0, ref0, 1000, prm, want_timing=True)
    (sh, sw), (rh, rw) = working_size(2400, 1700, 1000), working_size(700, 900, 1000)
    S, R = ctx.resize_u8c3(src0, sh, sw), ctx.resize_u8c3(ref0, rh, rw)
    ctx.pair_upload(S, R)
    keep = ctx.pair_run_levels(S.shape, R.shape, prm, want_color=True)
    h, w = keep["dims"][4][:2]
    exp, st = ctx.color_finish(keep["color"][4]["ab_nonlocal"], h, w, sh, sw, src0, prm, want_stages=True)
    assert np.array_equal(got, exp)
    assert tm["wls_iters"][4] == max(st["wls_iters"]) and tm["wls_level_ms"][4] > 0 and tm["wls_ms"] >= tm["wls_level_ms"][4]


def test_scale_and_limits():
    from caffemodel_io import synthetic_vgg19
    ws, bs = synthetic_vgg19(19)
    with nct.Context(0) as c:                                       # its own arena: the 24 MP buffers go back to the device with it
        c.vgg19_load_raw(ws, bs)
        src0 = c.resize_u8c3(synth.image(61, 600, 400), 6000, 4000)
        ref0 = synth.image(62, 800, 640)
        a, tm = c.process_pair_fullres(src0, ref0, 1000, _params(5), want_timing=True)
        assert a.shape == (6000, 4000, 3) and np.abs(a.astype(int) - src0.astype(int)).mean() > 1.0
        assert 0 < tm["wls_iters"][4] < 5000
        arena = c.counter(nct.CTR_ARENA_BYTES)
        assert arena > 6000 * 4000 * 48                             # at least the finish's six fp64 coefficient planes
        b = c.process_pair_fullres(src0, ref0, 1000, _params(5))
        assert np.array_equal(a, b)
        del a, b, src0
        strip = c.resize_u8c3(synth.image(63, 512, 64), 16384, 1000)       # working size 1000 x 61
        out = c.process_pair_fullres(strip, ref0, 1000, _params(5))
        assert out.shape == (16384, 1000, 3)
        del out, strip
        for shape in ((16385, 100), (100, 16385), (8193, 8192), (16384, 200)):
            img = np.zeros(shape + (3,), np.uint8)
            with pytest.raises(nct.NctError) as e:
                c.process_pair_fullres(img, ref0, 1000, _params(1))
            assert e.value.code == -2, shape
            with pytest.raises(nct.NctError) as e:
                c.process_pair_fullres(ref0, img, 1000, _params(1))
            assert e.value.code == -2, shape
        with pytest.raises(nct.NctError) as e:
            c.process_pair_fullres(ref0, ref0, 16, _params(1))
        assert e.value.code == -2


def test_cli_fullres(tmp_path, ctx):
    from caffemodel_io import synthetic_vgg19, write_caffemodel
    ws, bs = synthetic_vgg19(19)
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    big = synth.image(4, 1100, 700)
    Image.fromarray(big[..., ::-1].copy()).save(inp / "big.jpg", quality=90, subsampling=2)
    small = synth.image(5, 120, 160)
    Image.fromarray(small[..., ::-1].copy()).save(inp / "small.png")
    (inp / "pairs.txt").write_text("big.jpg small.png 2.0\nsmall.png big.jpg 1.0\n")
    dec = np.asarray(Image.open(inp / "big.jpg").convert("RGB"))[..., ::-1]
    ctx.vgg19_load_raw(ws, bs)
    prm = _params(1)
    outs = {}
    for tag, extra in (("full", ("-fullres", "1")), ("full2", ("-fullres", "1", "-inflight", "2")), ("plain", ("-fullres", "0"))):
        out = tmp_path / tag
        r = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-levels", "1", *extra], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(n for n in os.listdir(out) if n.endswith(".png")) == ["big_small_2.00.png", "small_big_1.00.png"]
        outs[tag] = {n: np.asarray(Image.open(out / n).convert("RGB"))[..., ::-1] for n in ("big_small_2.00.png", "small_big_1.00.png")}
    got = outs["full"]["big_small_2.00.png"]
    assert got.shape == (1100, 700, 3)
    prm.bds_weight = 2.0
    assert np.array_equal(got, ctx.process_pair_fullres(dec, small, 1000, prm))
    for n in outs["full"]:
        assert np.array_equal(outs["full"][n], outs["full2"][n]), n
    assert outs["plain"]["big_small_2.00.png"].shape == (1000, 636, 3)
    assert np.array_equal(outs["plain"]["big_small_2.00.png"], ctx.process_pair(ctx.resize_u8c3(dec, 1000, 636), small, prm))
    # the reverse pair: the content image is small, only the style image shrinks: the same file with or without -fullres
    assert np.array_equal(outs["full"]["small_big_1.00.png"], outs["plain"]["small_big_1.00.png"])
