"""Every form of the 3x3 conv kernel (k_vgg.hip: conv3x3_mfma2b_body) pinned one by one, through the device-pointer seams nct_conv3x3_dev / nct_conv3x3_pair_dev.

The body exists as four tile forms <WCO, CT> (waves along cout, 32-cout tiles per wave) — (1,2), (2,2), (2,1), (4,1) — chosen by nctk_conv3x3 from Cout and the number of
64-pixel wave tiles, each with three epilogues (planar store, channel-last store, fused 2x2/2 ceil-mode max-pool), plus the paired launch over two images. `form()` below
restates that dispatch, and the shape tables assert the form every case is meant to reach: a moved threshold fails here instead of silently testing another form.

Bars: bit equality with oracle/orc_vgg.c (same k order as the kernel), bit equality between the epilogues, and a derived float64 bound against tests/ref64.py:
|gpu - ref64| <= (9 Cin + 1) * 2^-24 * M with M = conv(|x|, |w|) + |b| — a chain of 9 Cin fused multiply-adds and one add, in any order; after pooling, the 2x2 ceil-mode
max of that bound map (a max moves by no more than its arguments). The oracle uses at most 0.11 of the bound on these shapes, so a wrong tap, channel or row cannot hide
inside it.

Which instantiation a launch takes is not reported by the library: profiles/conv_forms_kernels.md is the kernel-name / call-count table of this file under a kernel
trace, with all eight k_conv3x3_mfma2b<WCO, CT, POOL> and both k_conv3x3_mfma2b_pair<WCO, CT> instantiations in it."""
import ctypes as C
import functools
import numpy as np
import pytest
import ref64
import synth
from caffemodel_io import synthetic_vgg19

pytestmark = pytest.mark.gpu

PT1_BELOW = 128          # CONV_PT1_BELOW (k_vgg.hip)
U = 2.0 ** -24           # unit roundoff of float32


def cdiv(a, b):
    return (a + b - 1) // b


def form(cout, H, W, pool):
    """nctk_conv3x3's choice of <WCO, CT>"""
    wco = 2 if cout % 128 == 0 else 1
    ntiles = cdiv(W, 32) * cdiv(H, 2) if pool else cdiv(H * W, 64)
    full_blocks = cdiv(ntiles, 4 // wco) * (cout // (64 * wco))
    if full_blocks >= PT1_BELOW:
        return (2, 2) if wco == 2 else (1, 2)
    return (4, 1) if cout % 128 == 0 else (2, 1)


def pair_is_one_launch(cout, g1, g2):
    """nctk_conv3x3_pair's "both grids small" rule"""
    wco = 2 if cout % 128 == 0 else 1
    return all(cdiv(cdiv(h * w, 64), 4 // wco) * (cout // (64 * wco)) < PT1_BELOW for h, w in (g1, g2))


# (Cin, Cout, H, W), the form the case is meant to reach
PLAIN_CASES = [((6, 64, 179, 183), (1, 2)),        # 512 wave tiles, 128 workgroups: just over the threshold; odd number of channel pairs
               ((6, 128, 127, 129), (2, 2)),       # 256 tiles, 128 workgroups
               ((6, 256, 90, 91), (2, 2)),         # two cout blocks
               ((8, 64, 33, 47), (2, 1)),          # even number of channel pairs
               ((8, 128, 33, 47), (4, 1)),
               ((10, 256, 63, 65), (4, 1)),        # two cout blocks
               ((4, 64, 1, 40), (2, 1))]           # a one-row map
POOL_CASES = [((4, 64, 1, 40), (2, 1)),
              ((6, 64, 341, 65), (1, 2)),          # 3 x 171 tiles; the third column tile has one live column; odd H
              ((6, 128, 171, 65), (2, 2)),
              ((8, 64, 35, 65), (2, 1)),
              ((8, 128, 35, 65), (4, 1)),
              ((4, 64, 2, 32), (2, 1)),            # exactly one tile
              ((4, 64, 3, 33), (2, 1)),            # one column and one row over: clipped last row and last column
              ((4, 128, 7, 31), (4, 1))]           # one column short
# (Cin, Cout), image 1, image 2, one launch?
PAIR_CASES = [((8, 512), (11, 13), (9, 16), True),        # (4,1); 3 pixel blocks padded to 8
              ((8, 512), (40, 41), (11, 13), True),       # 26 blocks padded to 32
              ((8, 512), (11, 13), (40, 41), True),       # the other order
              ((6, 64), (33, 47), (19, 23), True),        # (2,1)
              ((6, 64), (179, 183), (33, 47), False)]     # the first image is not small: two launches
PAIR_OUTPUTS = {"hwc": ((0, 1), (0, 1)), "chw": ((1, 0), (1, 0)), "both": ((1, 1), (1, 1)), "mixed": ((1, 0), (0, 1))}       # per image (planar?, channel-last?)


def ids(cases):
    return ["x".join(map(str, c[0])) for c in cases]


def pair_ids(cases):
    return ["%dx%d_%dx%d_%dx%d" % (c[0] + c[1] + c[2]) for c in cases]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_shape_tables_reach_the_forms_they_name():
    for (cin, cout, H, W), f in PLAIN_CASES:
        assert form(cout, H, W, 0) == f, (cin, cout, H, W)
    for (cin, cout, H, W), f in POOL_CASES:
        assert form(cout, H, W, 1) == f, (cin, cout, H, W)
    assert {f for _, f in PLAIN_CASES} == {f for _, f in POOL_CASES} == {(1, 2), (2, 2), (2, 1), (4, 1)}
    for (cin, cout), g1, g2, one in PAIR_CASES:
        assert pair_is_one_launch(cout, g1, g2) == one and form(cout, *g1, 0)[1] == (1 if one else 2), (cout, g1, g2)
    assert {form(c[0][1], *c[1], 0) for c in PAIR_CASES if c[3]} == {(4, 1), (2, 1)}
    # the first two cases sit on the threshold: one workgroup fewer is the CT = 1 form
    assert form(64, 178, 182, 0) == (2, 1) and form(128, 127, 128, 0) == (4, 1)


@pytest.fixture(scope="module")
def gctx():
    import nct
    c = nct.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def inputs(cin, cout, H, W):
    """as in test_conv3x3_bit_exact: standard normal x and b, He-scaled weights, seeded per case"""
    rng = np.random.default_rng(cin * 1000 + W + 7919 * H + cout)
    x = rng.standard_normal((cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2 / (9 * cin))).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


_refs = {}


def refs(oracle, shape, relu):
    """(oracle map, float64 map, bound map) of a case, computed once and shared"""
    key = shape + (relu,)
    if key not in _refs:
        x, w, b = inputs(*shape)
        o = oracle.conv3x3(x, w, b, relu)
        y, m = ref64.conv3x3(x, w, b, relu)
        bound = (9 * shape[0] + 1) * U * m
        for a in (o, y, bound):
            a.setflags(write=False)
        _refs[key] = (o, y, bound)
    return _refs[key]


class Dev:
    """device buffers of one test, freed on exit; output buffers start as NaN so that an element no store reached cannot pass as the previous request's value"""
    def __init__(self, c):
        self.c, self.ptrs = c, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            self.c.dev_free(p)

    def up(self, arr):
        p = self.c.dev_upload(arr)
        self.ptrs.append(p)
        return p

    def planes(self, x):
        """the input of a layer: for an odd channel count the caller appends the zero plane (include/nct.h)"""
        if x.shape[0] & 1:
            x = np.concatenate([x, np.zeros((1,) + x.shape[1:], np.float32)])
        return self.up(x)

    def out(self, n):
        return self.up(np.full(n, np.nan, np.float32))


def conv_dev(c, x, w, b, relu, pool, want_chw, want_hwc):
    """nct_conv3x3_dev -> (planar map or None, channel-last map or None)"""
    cin, H, W = x.shape
    cout = w.shape[0]
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (H, W)
    with Dev(c) as d:
        dx, dw, db = d.planes(x), d.up(w), d.up(b)
        p_chw = d.out(cout * Ho * Wo) if want_chw else None
        p_hwc = d.out(cout * H * W) if want_hwc else None
        c.dev_call("conv3x3", dx, dw, db, cin, cout, H, W, int(relu), int(pool), p_chw, p_hwc)
        chw = c.dev_download(p_chw, (cout, Ho, Wo), np.float32) if want_chw else None
        hwc = c.dev_download(p_hwc, (H * W, cout), np.float32) if want_hwc else None
    return chw, hwc


def within(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    used = float((err / bound).max())
    print("%s: max |gpu - ref64| / bound = %.4f" % (what, used))
    assert np.isfinite(got).all() and (err <= bound).all(), "%s: %d elements outside the float64 bound (worst uses %.3f of it)" % (what, int((err > bound).sum()), used)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape,f", PLAIN_CASES, ids=ids(PLAIN_CASES))
def test_unpooled_planar_and_channel_last(gctx, oracle, shape, f, relu):
    """planar alone, channel-last alone (planar pointer null), both: the planar bits are the oracle's, the channel-last bits the planar map transposed, and neither
    depends on the other being asked for; the planar map lies within the float64 bound"""
    cin, cout, H, W = shape
    x, w, b = inputs(*shape)
    o, y, bound = refs(oracle, shape, relu)
    chw, none = conv_dev(gctx, x, w, b, relu, 0, True, False)
    none2, hwc = conv_dev(gctx, x, w, b, relu, 0, False, True)
    chw_b, hwc_b = conv_dev(gctx, x, w, b, relu, 0, True, True)
    assert none is None and none2 is None
    assert np.array_equal(bits(chw), bits(o)), "planar differs from the oracle: max abs diff %g" % np.nanmax(np.abs(chw - o))
    assert np.array_equal(bits(hwc), bits(chw.reshape(cout, H * W).T)), "channel-last differs from the transposed planar map"
    assert np.array_equal(bits(chw_b), bits(chw)) and np.array_equal(bits(hwc_b), bits(hwc)), "a store depends on whether the other one was requested"
    within(chw, y, bound, "conv %s %s" % (shape, f))
    within(hwc.T.reshape(cout, H, W), y, bound, "conv %s %s channel-last" % (shape, f))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("shape,f", POOL_CASES, ids=ids(POOL_CASES))
def test_pooled_epilogue(gctx, oracle, shape, f, relu):
    """the fused 2x2/2 ceil-mode max-pool: the bits of the oracle's conv followed by its pooling, within the pooled float64 bound"""
    x, w, b = inputs(*shape)
    o, y, bound = refs(oracle, shape, relu)
    got, _ = conv_dev(gctx, x, w, b, relu, 1, True, False)
    exp = oracle.maxpool2x2(o)
    assert got.shape == exp.shape
    assert np.array_equal(bits(got), bits(exp)), "pooled map differs from the oracle: max abs diff %g" % np.nanmax(np.abs(got - exp))
    within(got, ref64.maxpool2x2_ceil(y), ref64.maxpool2x2_ceil(bound), "conv + pool %s %s" % (shape, f))


def test_pool_and_refusals_of_the_launcher_stay(gctx):
    """no output at all, pool together with a channel-last output, Cout % 64: refused (NCT_ERR_INVALID), nothing launched"""
    import nct
    x, w, b = inputs(4, 64, 2, 32)
    with Dev(gctx) as d:
        dx, dw, db, po = d.planes(x), d.up(w), d.up(b), d.out(64 * 2 * 32)
        for args in ((dx, dw, db, 4, 64, 2, 32, 1, 0, None, None), (dx, dw, db, 4, 64, 2, 32, 1, 1, po, po), (dx, dw, db, 4, 96, 2, 32, 1, 0, po, None)):
            with pytest.raises(nct.NctError) as e:
                gctx.dev_call("conv3x3", *args)
            assert e.value.code == -2


def _delta_case():
    """delta weights at asymmetric taps on couts of both 32-cout tiles of a wave and of both cout blocks: cout -> (input plane, dy, dx), out(y, x) = in(y + dy, x + dx)"""
    taps = {5: (0, -1, 1), 37: (1, 1, 0), 69: (2, 0, -1), 101: (3, 1, 1)}
    w = np.zeros((128, 4, 3, 3), np.float32)
    for co, (ci, dy, dx) in taps.items():
        w[co, ci, dy + 1, dx + 1] = 1
    return taps, w


def _shifted(plane, dy, dx):
    H, W = plane.shape
    p = np.pad(plane, 1)
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


@pytest.mark.parametrize("H,W,pool", [(127, 129, 0), (171, 65, 1)], ids=["channel_last", "pooled"])
def test_conv_asymmetric_identity_check_new_epilogues(gctx, H, W, pool):
    """the transpose-detecting check of test_gpu_vgg.py::test_conv_asymmetric_identity_check for the channel-last and the pooled store of a CT = 2 form: every marked cout
    is the input plane moved by its tap's offset (pooled: the 2x2 ceil-mode max of that), every other cout exactly zero — a swapped tile, block, row or column shows"""
    assert form(128, H, W, pool) == (2, 2)
    taps, w = _delta_case()
    x = np.random.default_rng(3).standard_normal((4, H, W)).astype(np.float32)
    exp = np.zeros((128, H, W), np.float32)
    for co, (ci, dy, dx) in taps.items():
        exp[co] = _shifted(x[ci], dy, dx)
    b = np.zeros(128, np.float32)
    if pool:
        got, _ = conv_dev(gctx, x, w, b, False, 1, True, False)
        exp = ref64.maxpool2x2_ceil(exp).astype(np.float32)
    else:
        _, hwc = conv_dev(gctx, x, w, b, False, 0, False, True)
        got = hwc.T.reshape(128, H, W)
    for co in range(128):
        assert np.array_equal(got[co], exp[co]), "cout %d" % co          # value equality: an untouched cout may be +0 or -0


def pair_dev(c, case, relu, outputs):
    """nct_conv3x3_pair_dev -> [(planar or None, channel-last or None)] per image"""
    (cin, cout), g1, g2, _ = case
    x1, w, b = inputs(cin, cout, *g1)
    x2 = inputs(cin, cout, *g2)[0]
    with Dev(c) as d:
        dx = [d.planes(x1), d.planes(x2)]
        dw, db = d.up(w), d.up(b)
        p = [[d.out(cout * h * ww) if want else None for want in outputs[i]] for i, (h, ww) in enumerate((g1, g2))]
        c.dev_call("conv3x3_pair", dx[0], g1[0], g1[1], dx[1], g2[0], g2[1], dw, db, cin, cout, int(relu), p[0][0], p[1][0], p[0][1], p[1][1])
        res = []
        for i, (h, ww) in enumerate((g1, g2)):
            res.append((c.dev_download(p[i][0], (cout, h, ww), np.float32) if p[i][0] else None, c.dev_download(p[i][1], (h * ww, cout), np.float32) if p[i][1] else None))
    return res


def check_pair(c, oracle, case, relu, outputs):
    (cin, cout), g1, g2, _ = case
    x1, w, b = inputs(cin, cout, *g1)
    x2 = inputs(cin, cout, *g2)[0]
    res = pair_dev(c, case, relu, outputs)
    for i, (x, (h, ww)) in enumerate(((x1, g1), (x2, g2))):
        o = oracle.conv3x3(x, w, b, relu)
        s_chw, s_hwc = conv_dev(c, x, w, b, relu, 0, True, True)
        chw, hwc = res[i]
        assert (chw is not None) == bool(outputs[i][0]) and (hwc is not None) == bool(outputs[i][1])
        if chw is not None:
            assert np.array_equal(bits(chw), bits(o)), "image %d planar differs from the oracle" % (i + 1)
            assert np.array_equal(bits(chw), bits(s_chw)), "image %d planar differs from the single call" % (i + 1)
        if hwc is not None:
            assert np.array_equal(bits(hwc), bits(o.reshape(cout, h * ww).T)), "image %d channel-last differs from the oracle" % (i + 1)
            assert np.array_equal(bits(hwc), bits(s_hwc)), "image %d channel-last differs from the single call" % (i + 1)


@pytest.mark.parametrize("outputs", list(PAIR_OUTPUTS), ids=list(PAIR_OUTPUTS))
@pytest.mark.parametrize("case", PAIR_CASES, ids=pair_ids(PAIR_CASES))
def test_paired_launch(gctx, oracle, case, outputs):
    """two images of different geometry through one layer (the pipeline's conv5_1): every map equals two nct_conv3x3_dev calls and the oracle bit for bit, whichever
    outputs are asked for; the weights of image 1 serve both images, so the second image's inputs get weights and bias seeded for the first"""
    for relu in (True, False):
        check_pair(gctx, oracle, case, relu, PAIR_OUTPUTS[outputs])


def test_paired_launch_switched_off(oracle, monkeypatch):
    """NCT_CONV_PAIR=0: the two-launch path, the same bits"""
    import nct
    monkeypatch.setenv("NCT_CONV_PAIR", "0")
    with nct.Context(0) as c:
        check_pair(c, oracle, PAIR_CASES[0], True, PAIR_OUTPUTS["both"])


# ---------------------------------------------------------------- the forms inside a forward
IMG_HW = (192, 176)


@pytest.fixture(scope="module")
def weights():
    return synthetic_vgg19(19, bias_scale=0.05)


@pytest.fixture(scope="module")
def forward_refs(oracle, weights):
    """taps 1 and 2 of the image: the oracle's, the float64 reference's, and the float64 bound propagated layer by layer. A layer's computed output differs from the
    exact one by what its input's error E can do, conv(E, |w|), plus the rounding of its own sum, (9 Cin + 1) u (conv(|x| + E, |w|) + |b|); ReLU and max-pooling
    pass an error bound on unchanged (pooling: the window's max). The preprocess is one correctly rounded float32 subtraction in both, E = 0."""
    import torch
    import torch.nn.functional as F
    ws, bs = weights
    img = synth.image(7, *IMG_HW)
    o = oracle.vgg19_features(img, ws, bs, 2)
    r = ref64.vgg19_taps(img, ws, bs, 2)
    x = torch.from_numpy(np.ascontiguousarray((img.astype(np.float32) - np.asarray(ref64.VGG_MEAN_BGR, np.float32)).transpose(2, 0, 1), np.float64))[None]
    E = torch.zeros_like(x)
    bounds = []
    for i in range(3):                                                # conv1_1, conv1_2 (+ pool), conv2_1
        w, b = torch.from_numpy(np.asarray(ws[i], np.float64)), torch.from_numpy(np.asarray(bs[i], np.float64))
        n = 9 * w.shape[1] + 1
        E = F.conv2d(E, w.abs(), padding=1) + n * U * F.conv2d(x.abs() + E, w.abs(), b.abs(), padding=1)
        x = F.relu(F.conv2d(x, w, b, padding=1))
        if i in (0, 2):
            bounds.append(E[0].numpy().copy())
        if i == 1:
            x, E = F.max_pool2d(x, 2, 2, ceil_mode=True), F.max_pool2d(E, 2, 2, ceil_mode=True)
    assert np.array_equal(x[0].numpy(), r[1])                          # the walk above is the reference's
    return img, o, r, bounds


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_forward_to_tap2_reaches_the_ct2_forms(forward_refs, weights, monkeypatch, fuse):
    """nct_vgg19_features_hwc_dev to tap 2 on a 192 x 176 image: conv1_1 writes channel-last in the (1,2) form and, with the pool fused, conv1_2 pools in the (1,2) form.
    Both taps equal the oracle bit for bit, planar and channel-last (asked for together and channel-last alone), and lie within the float64 reference by the bound
    propagated layer by layer (forward_refs) — the GPU maps themselves, not only the oracle's."""
    import nct
    H, W = IMG_HW
    assert form(64, H, W, 0) == (1, 2) and form(64, H, W, 1) == (1, 2) and form(128, H // 2, W // 2, 0) == (4, 1)
    monkeypatch.setenv("NCT_CONV_POOL_FUSE", fuse)
    img, o, r, bounds = forward_refs
    ws, bs = weights
    shapes = [(64, H, W), (128, H // 2, W // 2)]
    with nct.Context(0) as c:
        c.vgg19_load_raw(ws, bs)
        with Dev(c) as d:
            dimg = d.up(img)
            chw, hwc, hwc_alone = ([d.out(int(np.prod(s))) for s in shapes] for _ in range(3))
            arr = lambda ps: (C.c_void_p * 5)(*(ps + [None] * 3))
            c.dev_call("vgg19_features_hwc", dimg, H, W, W * 3, 2, arr(chw), arr(hwc), None)
            c.dev_call("vgg19_features_hwc", dimg, H, W, W * 3, 2, None, arr(hwc_alone), None)
            for t, (cc, h, w) in enumerate(shapes):
                g = c.dev_download(chw[t], (cc, h, w), np.float32)
                assert np.array_equal(bits(g), bits(o[t])), "tap %d planar: max abs diff %g" % (t + 1, np.nanmax(np.abs(g - o[t])))
                for p in (hwc[t], hwc_alone[t]):
                    assert np.array_equal(bits(c.dev_download(p, (h * w, cc), np.float32)), bits(o[t].reshape(cc, h * w).T)), "tap %d channel-last" % (t + 1)
                within(g, r[t], bounds[t], "tap %d, fuse %s" % (t + 1, fuse))


def test_process_pair_is_the_same_with_and_without_the_paired_launch(weights, monkeypatch):
    """conv5_1 of the source and the reference in one launch or in two: the same result bytes"""
    import nct
    ws, bs = weights
    src, ref = synth.image(1000, 96, 80), synth.image(1001, 72, 104)
    got = {}
    for v in ("0", "1"):
        monkeypatch.setenv("NCT_CONV_PAIR", v)
        with nct.Context(0) as c:
            c.vgg19_load_raw(ws, bs)
            got[v] = c.process_pair(src, ref)
    assert got["0"].shape == src.shape and np.array_equal(got["0"], got["1"])
