"""The device-pointer seams of a level's correspondence block (include/nct.h "device-pointer seams", csrc/nct_dev.cpp; main.cu:204-316), each alone: against
tests/ref64.py, the float64 restatement of the reference's text, and bit for bit against the host form on the same data, whose parity with the oracle
(tests/test_gpu_correspondence.py) so carries over. test_gpu_pipeline.py::test_dev_seams_chain_equals_pipeline chains them on one image pair; here are the edge
grids, every nullable argument in both of its forms, the row stride, stream order and the refusals.

    seam                          form                        test
    nct_chw_to_hwc_dev                                        test_layout
    nct_hwc_to_chw_dev                                        test_layout
    nct_vgg19_features_dev        d_taps_chw[t] set / null    test_row_stride (taps 1, 2 set, 3..5 null); dims null / set
    nct_vgg19_features_hwc_dev    d_taps_chw, dims null / set test_row_stride
    nct_feat_normalize_dev        resp null / set             test_normalize, test_normalize_equal_norms
    nct_nnf_init_dev                                          test_nnf_init
    nct_nnf_upsample_dev                                      test_nnf_upsample
    nct_patchmatch_dev                                        test_patchmatch
    nct_patchmatch_bidir_dev      unit_norm 0 / 1             test_patchmatch_bidir
    nct_bds_vote_features_dev     pw null / set               test_votes
    nct_bds_vote_image_dev                                    test_votes
    nct_feature_distance_dev                                  test_feature_distance
    all of them                   back to back, recycled      test_stream_order
    all of them                   refused arguments           test_refusals

Not here: pointers off their natural alignment. The maps are read as float4 rows and the NNFs as words, so their alignment is part of the contract; the one
operand without any, the image rows of the VGG seams, is what test_row_stride misaligns."""
import ctypes as C

import numpy as np
import pytest

import nct
import ref64
import synth
from test_gpu_vs_ref64 import _check_pm
from test_ref64_oracle import (NORM_C, NORM_HW, NORM_MAP_TOL, SEAM_VOTE_C, SEAM_VOTE_GRIDS, _nnf_pair, _vote_image_agrees, check_feature_distance, check_normalize,
                               max_in_degree, norm_map)

pytestmark = pytest.mark.gpu


def to_hwc(chw):
    return np.ascontiguousarray(np.transpose(chw, (1, 2, 0)))


def to_chw(hwc):
    return np.ascontiguousarray(np.transpose(hwc, (2, 0, 1)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- layout
# one element; odd everything; one channel tile with a part-filled pixel tile; two channel tiles, the second with one channel; several tiles each way; C past 512;
# and the long axis: 1025 * 2049 pixels are 65 633 tiles of 32, which nct_hwc_to_chw_dev's launch carries on grid.y — past 65 535; the runtime takes it
LAYOUT_SHAPES = [(1, 1, 1), (3, 5, 7), (4, 1, 33), (33, 1, 31), (64, 9, 7), (513, 3, 11), (4, 1025, 2049)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_layout(ctx, shape):
    """Both layout changes move every 32-bit word untouched: random bit patterns — NaNs of every payload, infinities, denormals, -0.0 among them, the named ones
    planted — equal np.transpose as uint32."""
    Cc, H, W = shape
    n = Cc * H * W
    x = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0x00000001], np.uint32)   # -0, +-inf, quiet / signalling NaNs, a denormal
    x[np.arange(special.size) * 7 % n] = special
    with ctx.blocks() as b:
        src, dst = b.up(x), b.new(4 * n)
        ctx.dev_call("chw_to_hwc", src, dst, Cc, H, W)
        assert np.array_equal(ctx.dev_download(dst, (H, W, Cc), np.uint32), np.transpose(x.reshape(Cc, H, W), (1, 2, 0)))
        ctx.dev_call("hwc_to_chw", src, dst, Cc, H, W)
        assert np.array_equal(ctx.dev_download(dst, (Cc, H, W), np.uint32), np.transpose(x.reshape(H, W, Cc), (2, 0, 1)))


# ---------------------------------------------------------------- normalise, matching error
def dev_normalize(c, f, want_resp=False):
    """nct_feat_normalize_dev on a CHW host map -> CHW (and the response), in the host form's shape"""
    Cc, H, W = f.shape
    with c.blocks() as b:
        src, dst, rp = b.up(to_hwc(f)), b.new(4 * f.size), b.new(4 * H * W) if want_resp else None
        c.dev_call("feat_normalize", src, dst, rp, Cc, H, W)
        out = to_chw(c.dev_download(dst, (H, W, Cc), np.float32))
        return (out, c.dev_download(rp, (H, W), np.float32)) if want_resp else out


def dev_feature_distance(c, a, bmap):
    Cc, H, W = a.shape
    with c.blocks() as b:
        pa, pb, err = b.up(to_hwc(a)), b.up(to_hwc(bmap)), b.new(4 * H * W)
        c.dev_call("feature_distance", pa, pb, err, Cc, H, W)
        return c.dev_download(err, (H, W), np.float32)


@pytest.mark.parametrize("Cc", NORM_C)
def test_normalize(ctx, Cc):
    """Over the HW column of the table (test_ref64_oracle.py: NORM_C, NORM_HW), with and without a dead pixel: the map and the response within NORM_MAP_TOL /
    NORM_RESP_TOL of ref64 (calibrated on the CPU against the oracle, never here); a zero pixel is NaN over its C values, 0 in the response, and nothing else
    is NaN; the map has the same bits whether or not the response is asked for; both outputs have the bits of nct_feat_normalize."""
    for HW in NORM_HW:
        for dead in ((False, True) if HW > 1 else (False,)):
            dm, dr = check_normalize(lambda f, want_resp: dev_normalize(ctx, f, want_resp), Cc, HW, dead)
            print("normalize C=%d HW=%d dead=%d: map %.3g response %.3g" % (Cc, HW, dead, dm, dr))
            f = norm_map(Cc, HW, dead=dead)
            got, resp = dev_normalize(ctx, f, True)
            host, hresp = ctx.feat_normalize(f, want_resp=True)
            assert same_bits(got, dev_normalize(ctx, f)) and same_bits(got, host) and same_bits(resp, hresp), (Cc, HW, dead)


def test_normalize_equal_norms(ctx):
    """max = min: the reference's text (GeneralizedPatchMatch.cu:270-271) shifts every norm to 0 and scales by 1 / 0, so the response is NaN at every pixel
    (ref64.response); the normalised map is unaffected."""
    f = np.tile(synth.features(5, 20, 1, 1), (1, 3, 5)) * np.where(np.arange(15).reshape(1, 3, 5) % 2, -1, 1).astype(np.float32)
    got, resp = dev_normalize(ctx, f, True)
    assert np.isnan(resp).all() and np.isnan(ref64.response(f)).all()
    assert np.abs(got - ref64.normalize(f)).max() <= NORM_MAP_TOL
    host, hresp = ctx.feat_normalize(f, want_resp=True)
    assert same_bits(got, host) and np.isnan(hresp).all()


@pytest.mark.parametrize("Cc", NORM_C)
def test_feature_distance(ctx, Cc):
    """unit vectors (normalised by the seam) over the HW column: within FEATURE_DISTANCE_TOL of ref64, the bits of nct_feature_distance"""
    for HW in NORM_HW:
        d = check_feature_distance(lambda f: dev_normalize(ctx, f), lambda a, b: dev_feature_distance(ctx, a, b), Cc, HW)
        print("feature_distance C=%d HW=%d: %.3g" % (Cc, HW, d))
        a, b = dev_normalize(ctx, norm_map(Cc, HW, 1)), dev_normalize(ctx, norm_map(Cc, HW, 2))
        assert same_bits(dev_feature_distance(ctx, a, b), ctx.feature_distance(a, b)), (Cc, HW)


# ---------------------------------------------------------------- NNF
@pytest.mark.parametrize("dims", [(2, 2, 5, 3), (2, 2, 1, 1), (17, 23, 31, 17)])
def test_nnf_init(ctx, dims):
    ah, aw, bh, bw = dims
    with ctx.blocks() as b:
        nnf = b.new(4 * ah * aw)
        ctx.dev_call("nnf_init", nnf, ah, aw, bh, bw)
        got = ctx.dev_download(nnf, (ah, aw), np.uint32)
    assert np.array_equal(got, ref64.nnf_init(ah, aw, bh, bw)) and np.array_equal(got, ctx.nnf_init(ah, aw, bh, bw))


# (ah_half, aw_half, ah, aw, bh, bw): the cases of test_gpu_vs_ref64.py::test_nnf_upsample_vs_ref64 and one pixel to a 2 x 2 map
@pytest.mark.parametrize("dims", [(44, 44, 88, 88, 88, 88), (88, 88, 175, 175, 175, 175), (29, 43, 57, 85, 75, 120), (57, 85, 113, 170, 150, 240), (16, 16, 32, 32, 32, 32),
                                  (1, 1, 2, 2, 3, 3)])
def test_nnf_upsample(ctx, dims):
    ahh, awh, ah, aw, bh, bw = dims
    half = synth.random_nnf(5, ahh, awh, (bh + 1) // 2, (bw + 1) // 2)
    with ctx.blocks() as b:
        ph, nnf = b.up(half), b.new(4 * ah * aw)
        ctx.dev_call("nnf_upsample", ph, nnf, ah, aw, bh, bw, ahh, awh)
        got = ctx.dev_download(nnf, (ah, aw), np.uint32)
    assert np.array_equal(got, ref64.nnf_upsample(half, ah, aw, bh, bw)) and np.array_equal(got, ctx.nnf_upsample(half, ah, aw, bh, bw))


# ---------------------------------------------------------------- PatchMatch
# (ah, aw, bh, bw): a 2 x 2 query map; odd; several query tiles at every C; a one-row query map against a one-column map (pm_run takes both)
PM_GRIDS = [(2, 2, 5, 3), (7, 5, 9, 11), (17, 23, 31, 17), (1, 9, 3, 1)]


def pm_maps(c, b, Cc, dims, dead=False):
    """two feature maps normalised on the device: their blocks (HWC) and host copies (CHW)"""
    ah, aw, bh, bw = dims
    fa, fb = synth.features(31, Cc, ah, aw), synth.features(32, Cc, bh, bw)
    if dead:
        fa[:, ah // 2, aw // 3] = 0; fa[:, ah - 1, aw - 1] = 0; fb[:, bh // 3: bh // 3 + 2, bw // 2] = 0; fb[:, 0, 0] = 0
    out = []
    for f in (fa, fb):
        raw, nrm = b.up(to_hwc(f)), b.new(4 * f.size)
        c.dev_call("feat_normalize", raw, nrm, None, *f.shape)
        out += [nrm, to_chw(c.dev_download(nrm, f.shape[1:] + (Cc,), np.float32))]
    return out


# C = 8: the generic instantiation; 64: the lane-interleaved copies; 128 and 512: two of the tiled ones
@pytest.mark.parametrize("Cc", [8, 64, 128, 512])
def test_patchmatch(ctx, Cc):
    """nct_patchmatch_dev, one field from a random one, 3 iterations, rs_max 8: what test_gpu_vs_ref64.py::_check_pm asks (the distance is ref64's at the returned
    match within 1e-5, NaN exactly where a tap is a dead pixel, matches inside B, no pixel worse than it began), and the bits of nct_patchmatch on the CHW copies.
    The 17 x 23 grid has dead feature pixels in both maps."""
    for dims in PM_GRIDS:
        ah, aw, bh, bw = dims
        with ctx.blocks() as b:
            pa, a, pb, bm = pm_maps(ctx, b, Cc, dims, dead=dims == PM_GRIDS[2])
            nnf0 = synth.random_nnf(11, ah, aw, bh, bw)
            pn, pd = b.up(nnf0), b.new(4 * ah * aw)
            ctx.dev_call("patchmatch", pa, pb, Cc, ah, aw, bh, bw, 3, 3, 8, 11, pn, pd)
            nnf, d = ctx.dev_download(pn, (ah, aw), np.uint32), ctx.dev_download(pd, (ah, aw), np.float32)
        if dims == PM_GRIDS[2]:
            assert np.isnan(a).any() and np.isnan(bm).any() and np.isnan(d).any()
        _check_pm(a, bm, nnf0, nnf, d)
        hn, hd = ctx.patchmatch(a, bm, nnf0, iters=3, rs_max=8, seed=11)
        assert np.array_equal(nnf, hn) and same_bits(d, hd), dims


@pytest.mark.parametrize("Cc,dims", [(64, (17, 23, 31, 17)), (512, (7, 5, 9, 11)), (128, (1, 9, 3, 1))])
def test_patchmatch_bidir(ctx, oracle, Cc, dims):
    """nct_patchmatch_bidir_dev on unit vectors: unit_norm 0 and 1 give the same fields and bit-identical distances in both directions, those of the oracle's two
    single-direction runs with the same seeds (as test_gpu_correspondence.py::test_patchmatch_bidir_bit_exact compares the pipeline's launches)."""
    ah, aw, bh, bw = dims
    sa, sb = 77, 77 ^ 0x5bd1e995
    ann0, bnn0 = synth.random_nnf(1, ah, aw, bh, bw), synth.random_nnf(2, bh, bw, ah, aw)
    runs = []
    with ctx.blocks() as b:
        pa, a, pb, bm = pm_maps(ctx, b, Cc, dims)
        for unit in (0, 1):
            an, bn, ad, bd = b.up(ann0), b.up(bnn0), b.new(4 * ah * aw), b.new(4 * bh * bw)
            ctx.dev_call("patchmatch_bidir", pa, pb, Cc, ah, aw, bh, bw, 3, 3, 8, sa, sb, an, ad, bn, bd, unit)
            runs.append((ctx.dev_download(an, (ah, aw), np.uint32), ctx.dev_download(ad, (ah, aw), np.float32),
                         ctx.dev_download(bn, (bh, bw), np.uint32), ctx.dev_download(bd, (bh, bw), np.float32)))
    exp = oracle.patchmatch(a, bm, ann0, iters=3, rs_max=8, seed=sa) + oracle.patchmatch(bm, a, bnn0, iters=3, rs_max=8, seed=sb)
    for unit, got in enumerate(runs):
        for g, e in zip(got, exp):
            assert same_bits(g, e), (unit, dims)


# ---------------------------------------------------------------- votes
VOTE_KINDS = ("random", "collapsed", "border", "collapsed_b")


@pytest.mark.parametrize("weights", [(1.0, 2.0), (2.0, 1.0)])
@pytest.mark.parametrize("Cc", SEAM_VOTE_C)
def test_votes(ctx, Cc, weights):
    """Both vote seams over SEAM_VOTE_GRIDS and the four field kinds — collapsed_b, a collapsed R -> S field, is the hub pass's: more than 130 sources on one
    target at the second grid — against ref64 with the tolerances of test_gpu_vs_ref64.py::test_votes_vs_ref64 (test_ref64_oracle.py::test_votes_collapsed_b:
    the oracle keeps inside them on collapsed_b too); the feature vote has the same bits with and without pw; all outputs have the bits of the host forms."""
    wc, wp = weights
    for (ah, aw, bh, bw) in SEAM_VOTE_GRIDS:
        pin = synth.features(7, Cc, bh, bw)
        ia, ib = synth.image(1, ah, aw), synth.image(2, bh, bw)
        for kind in VOTE_KINDS:
            ann, bnn = _nnf_pair(kind, 3, 4, ah, aw, bh, bw)
            if kind == "collapsed_b" and bh * bw >= 260:
                assert max_in_degree(bnn, ah, aw) >= 130
            with ctx.blocks() as b:
                pa, pb, pp, pi = b.up(ann), b.up(bnn), b.up(to_hwc(pin)), b.up(ib)
                out, out2, pw, img = b.new(4 * Cc * ah * aw), b.new(4 * Cc * ah * aw), b.new(4 * ah * aw), b.new(3 * ah * aw)
                ctx.dev_call("bds_vote_features", pa, pb, pp, out, None, Cc, ah, aw, bh, bw, 3, wc, wp)
                ctx.dev_call("bds_vote_features", pa, pb, pp, out2, pw, Cc, ah, aw, bh, bw, 3, wc, wp)
                ctx.dev_call("bds_vote_image", pi, pa, pb, ah, aw, bh, bw, 3, wc, wp, img)
                got, got2 = (to_chw(ctx.dev_download(p, (ah, aw, Cc), np.float32)) for p in (out, out2))
                gpw, gi = ctx.dev_download(pw, (ah, aw), np.float32), ctx.dev_download(img, (ah, aw, 3), np.uint8)
            what = (kind, ah, aw, bh, bw)
            exp, epw = ref64.vote_features(ann, bnn, pin, wc, wp)
            assert np.allclose(got, exp, rtol=1e-5, atol=1e-6), what
            assert np.allclose(gpw, epw, rtol=1e-5, atol=1e-12), what
            ei, v = ref64.vote_image(ia, ib, ann, bnn, wc, wp, want_float=True)
            assert _vote_image_agrees(gi, ei, v), what
            host, hpw = ctx.bds_vote_features(ann, bnn, pin, wc, wp, want_pw=True)
            assert same_bits(got, got2) and same_bits(got, host) and same_bits(gpw, hpw), what
            assert np.array_equal(gi, ctx.bds_vote_image(ia, ib, ann, bnn, wc, wp)), what


# ---------------------------------------------------------------- row stride
@pytest.fixture(scope="module")
def vgg():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


def test_row_stride(ctx, vgg):
    """A 17 x 19 image in rows of 3 * 19 + 5 bytes — an odd pitch, so every row but the first starts off any alignment — with 0xFF between the rows: taps 1 and 2 of
    nct_vgg19_features_dev (planar), of nct_vgg19_features_hwc_dev (channel-last alone, and beside the planar maps) and of nct_vgg19_features have the bits of
    the packed image's."""
    ctx.vgg19_load_raw(*vgg)
    h, w, stride = 17, 19, 3 * 19 + 5
    img = synth.image(3, h, w)
    want = ctx.vgg19_features(img, 2)
    shapes = [(64, 17, 19), (128, 9, 10)]
    assert [t.shape for t in want] == shapes
    for t, e in zip(ctx.vgg19_features(img, 2, stride=stride), want):
        assert same_bits(t, e)
    buf = np.full((h, stride), 0xFF, np.uint8)
    buf[:, :3 * w] = img.reshape(h, 3 * w)
    with ctx.blocks() as b:
        d_img = b.up(buf)
        chw, hwc, chw2 = ([b.new(4 * int(np.prod(s))) for s in shapes] for _ in range(3))
        arr = lambda ps: (C.c_void_p * 5)(*(ps + [None] * 3))
        dims = np.zeros(15, np.int32)
        ctx.dev_call("vgg19_features", d_img, h, w, stride, 2, arr(chw), dims.ctypes.data)
        ctx.dev_call("vgg19_features_hwc", d_img, h, w, stride, 2, None, arr(hwc), None)
        dims2 = np.zeros(15, np.int32)
        ctx.dev_call("vgg19_features_hwc", d_img, h, w, stride, 2, arr(chw2), arr(hwc), dims2.ctypes.data)
        for t, s in enumerate(shapes):
            assert same_bits(ctx.dev_download(chw[t], s, np.float32), want[t]) and same_bits(ctx.dev_download(chw2[t], s, np.float32), want[t]), t
            assert same_bits(to_chw(ctx.dev_download(hwc[t], s[1:] + s[:1], np.float32)), want[t]), t
        assert dims[:6].tolist() == dims2[:6].tolist() == [64, 17, 19, 128, 9, 10]


# ---------------------------------------------------------------- stream order
def test_stream_order(ctx):
    """Two different chains enqueued back to back with no synchronisation between them — normalise, PatchMatch at C = 64 (its lane-interleaved copies) and the
    matching error; then normalise with the response (its norms and extremes), both votes (their inverse maps) — while blocks of the first go back and blocks of equal size
    are taken for the second: one download at the end has the bytes of each chain run alone. The seams' temporaries and the recycled blocks follow stream order."""
    Cc, (ah, aw, bh, bw) = 64, (17, 23, 31, 17)
    fa, fb = synth.features(41, Cc, ah, aw), synth.features(42, Cc, bh, bw)
    nnf0 = synth.random_nnf(11, ah, aw, bh, bw)
    ann, bnn = _nnf_pair("collapsed_b", 3, 4, ah, aw, bh, bw)
    ib = synth.image(2, bh, bw)
    na, nb = 4 * Cc * ah * aw, 4 * Cc * bh * bw

    def chain1(b, u):
        a_n, b_n, d, err = b.new(na), b.new(nb), b.new(4 * ah * aw), b.new(4 * ah * aw)
        ctx.dev_call("feat_normalize", u["fa"], a_n, None, Cc, ah, aw); ctx.dev_call("feat_normalize", u["fb"], b_n, None, Cc, bh, bw)
        ctx.dev_call("patchmatch", a_n, b_n, Cc, ah, aw, bh, bw, 3, 3, 8, 11, u["nnf"], d)
        ctx.dev_call("feature_distance", a_n, u["fa"], err, Cc, ah, aw)
        b.free(a_n); b.free(b_n)                                  # back to the arena while the kernels above are still to run
        return lambda: [ctx.dev_download(u["nnf"], (ah, aw), np.uint32), ctx.dev_download(d, (ah, aw), np.float32), ctx.dev_download(err, (ah, aw), np.float32)]

    def chain2(b, u):
        b_n, voted, resp, pw, img = b.new(nb), b.new(na), b.new(4 * bh * bw), b.new(4 * ah * aw), b.new(3 * ah * aw)      # the sizes chain1 gave back
        ctx.dev_call("feat_normalize", u["fb"], b_n, resp, Cc, bh, bw)
        ctx.dev_call("bds_vote_features", u["ann"], u["bnn"], b_n, voted, pw, Cc, ah, aw, bh, bw, 3, 1.0, 2.0)
        ctx.dev_call("bds_vote_image", u["img"], u["ann"], u["bnn"], ah, aw, bh, bw, 3, 1.0, 2.0, img)
        return lambda: [ctx.dev_download(voted, (ah, aw, Cc), np.float32), ctx.dev_download(resp, (bh, bw), np.float32), ctx.dev_download(pw, (ah, aw), np.float32),
                        ctx.dev_download(img, (ah, aw, 3), np.uint8)]

    def uploads(b):
        return {"fa": b.up(to_hwc(fa)), "fb": b.up(to_hwc(fb)), "nnf": b.up(nnf0), "ann": b.up(ann), "bnn": b.up(bnn), "img": b.up(ib)}

    alone = []
    for chain in (chain1, chain2):
        with ctx.blocks() as b:
            alone.append(chain(b, uploads(b))())
    with ctx.blocks() as b:
        u = uploads(b)                                            # every upload waits for the stream: all of them in front of the chains
        get1 = chain1(b, u)
        get2 = chain2(b, u)
        both = [get1(), get2()]
    for g, e in zip(both[0] + both[1], alone[0] + alone[1]):
        assert same_bits(g, e)
    assert not np.array_equal(both[0][0], nnf0) and np.isfinite(both[1][0]).all()


# ---------------------------------------------------------------- refusals
BIG = 4096
# a valid call of every seam on tiny blocks: argument names in the symbol's order; the names in `dims` take BIG and 0 / -1 in turn
SEAMS = {
    "chw_to_hwc": (["src", "dst", "C", "H", "W"], {"C": 4, "H": 3, "W": 5}),
    "hwc_to_chw": (["src", "dst", "C", "H", "W"], {"C": 4, "H": 3, "W": 5}),
    "vgg19_features": (["img", "h", "w", "stride", "tap", "taps", "dims"], {"h": 17, "w": 19, "stride": 57, "tap": 1, "dims": None}),
    "vgg19_features_hwc": (["img", "h", "w", "stride", "tap", "none", "taps", "dims"], {"h": 17, "w": 19, "stride": 57, "tap": 1, "dims": None, "none": None}),
    "feat_normalize": (["src", "dst", "resp", "C", "H", "W"], {"C": 4, "H": 3, "W": 5}),
    "nnf_init": (["nnf", "ah", "aw", "bh", "bw"], {"ah": 3, "aw": 5, "bh": 4, "bw": 3}),
    "nnf_upsample": (["half", "nnf", "ah", "aw", "bh", "bw", "ahh", "awh"], {"ah": 3, "aw": 5, "bh": 4, "bw": 3, "ahh": 2, "awh": 3}),
    "patchmatch": (["a", "b", "C", "ah", "aw", "bh", "bw", "patch", "iters", "rs", "seed", "nnf", "dist"],
                   {"C": 4, "ah": 3, "aw": 5, "bh": 4, "bw": 3, "patch": 3, "iters": 1, "rs": 2, "seed": 1}),
    "patchmatch_bidir": (["a", "b", "C", "ah", "aw", "bh", "bw", "patch", "iters", "rs", "seed", "seed2", "nnf", "dist", "bnn", "bdist", "unit"],
                         {"C": 4, "ah": 3, "aw": 5, "bh": 4, "bw": 3, "patch": 3, "iters": 1, "rs": 2, "seed": 1, "seed2": 2, "unit": 0}),
    "bds_vote_features": (["nnf", "bnn", "b", "dst", "resp", "C", "ah", "aw", "bh", "bw", "patch", "wc", "wp"],
                          {"C": 4, "ah": 3, "aw": 5, "bh": 4, "bw": 3, "patch": 3, "wc": 1.0, "wp": 2.0}),
    "bds_vote_image": (["img", "nnf", "bnn", "ah", "aw", "bh", "bw", "patch", "wc", "wp", "out"], {"ah": 3, "aw": 5, "bh": 4, "bw": 3, "patch": 3, "wc": 1.0, "wp": 2.0}),
    "feature_distance": (["src", "a", "dist", "C", "H", "W"], {"C": 4, "H": 3, "W": 5}),
}
NULLABLE = ("resp", "dims", "none", "taps")
FIELD_DIMS = ("ah", "aw", "bh", "bw")
# the arguments each seam writes: compared after every refusal with the bytes of the valid call made before the first one
OUTPUTS = {"chw_to_hwc": ["dst"], "hwc_to_chw": ["dst"], "vgg19_features": ["tap0"], "vgg19_features_hwc": ["tap0"], "feat_normalize": ["dst", "resp"], "nnf_init": ["nnf"],
           "nnf_upsample": ["nnf"], "patchmatch": ["nnf", "dist"], "patchmatch_bidir": ["nnf", "dist", "bnn", "bdist"], "bds_vote_features": ["dst", "resp"],
           "bds_vote_image": ["out"], "feature_distance": ["dist"]}


def refusal_cases(name):
    """(label, changed arguments) of every refusal of a seam; the checks stand in nct_dev.cpp in front of the launcher's first reservation and launch"""
    args, vals = SEAMS[name]
    cases = [("null " + a, {a: None}) for a in args if a not in vals and a not in NULLABLE]
    for d in [a for a in args if a in ("H", "W", "h", "w", "ahh", "awh") + FIELD_DIMS]:
        cases += [(d + " = 0", {d: 0}), (d + " = -1", {d: -1})]
        if d in FIELD_DIMS or d in ("h", "w", "ahh", "awh"):
            cases.append((d + " = 4096", {d: BIG}))
    if "C" in vals:
        cases += [("C = 0", {"C": 0}), ("C = -4", {"C": -4})]
        if name in ("chw_to_hwc", "hwc_to_chw"):
            cases += [("H W past int", {"C": 1, "H": 46341, "W": 46341}), ("C H W past int", {"C": 512, "H": 2048, "W": 2048})]
        else:
            cases += [("C = 6", {"C": 6}), ("C = 1", {"C": 1})]
        if name in ("feat_normalize", "feature_distance"):
            cases += [("H W past int", {"H": 65536, "W": 65536}), ("C H W past int", {"C": 512, "H": 2048, "W": 2048})]
        if name == "bds_vote_features":
            cases.append(("C = 516", {"C": 516}))
    if "patch" in vals:
        cases += [("patch = 5", {"patch": 5}), ("patch = 1", {"patch": 1})]
    if "iters" in vals:
        cases += [("iters = -1", {"iters": -1}), ("rs_max = -1", {"rs": -1})]
    if "stride" in vals:
        cases += [("stride = 3 w - 1", {"stride": 56}), ("tap = 0", {"tap": 0}), ("tap = 6", {"tap": 6})]
    if name == "nnf_upsample":
        cases.append(("nnf_half == nnf", {"half": "nnf"}))
    if name == "nnf_init":
        cases += [("ah = 1", {"ah": 1}), ("aw = 1", {"aw": 1})]
    return cases


def test_refusals(vgg):
    """Every seam of the family refuses a null operand, C = 0 or not a multiple of 4 (normalise, matching error, PatchMatch, the feature vote; > 512 there), a
    dimension <= 0, a dimension >= 4096 wherever an NNF is read or written (and on the VGG image), patch != 3, negative iters / rs_max, a stride below a row, a
    deepest tap outside 1..5, nnf_half == nnf, a one-row query map for the init, and sizes past the launchers' ints: NCT_ERR_INVALID, a message that begins with the
    entry point's name, the arena's byte count where it was. After each refusal the same seam, called rightly on the same context, writes the bytes it wrote
    before. nct_bds_vote_features and nct_bds_vote_image, the host forms, refuse a dimension of 4096 likewise. A context of the test's own, so that the count is its alone; the count grows only when a reservation finds no free block of its size (the large
    dimensions would), so that the checks stand in front of every reservation is first of all what reading nct_dev.cpp shows."""
    f = synth.features(1, 4, 3, 5)
    host = {"src": to_hwc(f), "a": to_hwc(synth.features(2, 4, 3, 5)), "b": to_hwc(synth.features(3, 4, 4, 3)), "nnf": synth.random_nnf(1, 3, 5, 4, 3),
            "bnn": synth.random_nnf(2, 4, 3, 3, 5), "half": synth.random_nnf(3, 2, 3, 2, 2), "img": synth.image(3, 17, 19)}
    out_bytes = {"dst": 4 * 60, "resp": 4 * 15, "dist": 4 * 15, "bdist": 4 * 12, "out": 3 * 15, "tap0": 4 * 64 * 17 * 19}
    n_refused = 0
    with nct.Context(0) as c:
        c.vgg19_load_raw(*vgg)
        with c.blocks() as b:
            dev = {k: b.up(v) for k, v in host.items()}
            dev.update({k: b.new(n) for k, n in out_bytes.items()})
            dev["taps"] = (C.c_void_p * 5)(dev["tap0"], None, None, None, None)
            size = dict(out_bytes, nnf=4 * 15, bnn=4 * 12)

            def call(name, change):
                args, vals = SEAMS[name]
                v = dict(dev, **vals)
                v.update({k: (v[x] if isinstance(x, str) else x) for k, x in change.items()})
                for k in ("nnf", "bnn"):                          # PatchMatch works in place: every call starts from the same field
                    c.dev_call("nnf_upsample", dev["half"], dev[k], *((3, 5, 4, 3) if k == "nnf" else (4, 3, 3, 5)), 2, 3)
                return getattr(c._l, "nct_" + name + "_dev")(c._h, *[v[a] for a in args])

            def outputs(name):
                return [c.dev_download(dev[k], (size[k],), np.uint8) for k in OUTPUTS[name]]

            for name in SEAMS:
                assert call(name, {}) == 0, (name, c._l.nct_last_error(c._h).decode())
                good = outputs(name)
                for label, change in refusal_cases(name):
                    held = c.counter(nct.CTR_ARENA_BYTES)
                    rc = call(name, change)
                    msg = c._l.nct_last_error(c._h).decode()
                    assert rc == -2 and msg.startswith(name + "_dev: "), (name, label, rc, msg)
                    assert c.counter(nct.CTR_ARENA_BYTES) == held, (name, label)
                    n_refused += 1
                    assert call(name, {}) == 0, (name, label)
                    for g, e in zip(outputs(name), good):
                        assert np.array_equal(g, e), (name, label)
        # the host forms of the votes take the same field dimensions (nctk_bds_vote_*; repeated in nct_api.cpp in front of their reservations)
        wide, tall = np.zeros((1, BIG), np.uint32), np.zeros((BIG, 1), np.uint32)
        for ann, bnn, pin in ((wide, host["bnn"], synth.features(3, 4, 4, 3)), (host["nnf"], tall, synth.features(3, 4, BIG, 1))):
            held = c.counter(nct.CTR_ARENA_BYTES)
            for vote, who in ((lambda: c.bds_vote_features(ann, bnn, pin), "bds_vote_features"),
                              (lambda: c.bds_vote_image(np.zeros(ann.shape + (3,), np.uint8), np.zeros(bnn.shape + (3,), np.uint8), ann, bnn), "bds_vote_image")):
                with pytest.raises(nct.NctError) as e:
                    vote()
                assert e.value.code == -2 and who + ": dims out of range" in str(e.value)
            assert c.counter(nct.CTR_ARENA_BYTES) == held
    assert n_refused >= 190, n_refused
