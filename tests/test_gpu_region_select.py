"""Region selection from strokes (SPEC §6.16) on the GPU: nct_feat_quantize[_dev] and nct_region_score[_dev] against the numpy rule (tests/region_select_ref.py), the
whole call with all four stages for the host and the device form, its compositions with the region setters of a pair and of a tracked and snapped sequence, the arena,
the refusals. Every comparison is equality of bytes.

The score kernel's edges (k_region_select.hip), all hit by SCORE_CASES: a workgroup owns 128 query cells (cells 127 / 128 / 129 and 1000 = 7 tiles + 104); the seeds
are ONE list, inside first, walked 64 at a time (n_in + n_out = 64, 65, 128, 129, 130, 365), so a class border may fall inside a chunk (5 + 1, 64 + 1, 63 + 1, 65 + 65)
or on its edge (64 + 65); channels are staged 64 at a time (C = 64: one stage, 512: eight, 68: a tail of 4, 4: a tail alone)."""
import ctypes as C

import numpy as np
import pytest

import nct
import region_select_ref as sel
import region_snap_ref as rs
import seq_mc_ref
import synth

pytestmark = pytest.mark.gpu

INVALID, STATE = -2, -5
H, W = 56, 64
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def sources(oracle, weights):
    """per size of sel.SIZES: the source and the oracle's five taps of it, computed once"""
    out = {}
    for h, w in sel.SIZES:
        src = sel.call_source(h, w)
        out[(h, w)] = (src, oracle.vgg19_features(src, *weights, deepest_tap=5))
    return out


def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def raw_refused(c, fn, args, code, word):
    rc = getattr(c._l, fn)(c._h, *args)
    msg = c._l.nct_last_error(c._h).decode()
    assert rc == code and word in msg, (fn, rc, msg)


# ---------------------------------------------------------------- nct_feat_quantize
@pytest.mark.parametrize("Cc", [64, 128, 512])
@pytest.mark.parametrize("grid", [(1, 1), (3, 5), (17, 19)])
def test_feat_quantize(ctx, oracle, Cc, grid):
    gh, gw = grid
    f = synth.features(40 + Cc + gh, Cc, gh, gw, smooth=False)
    variants = [f]
    if gh * gw == 1:
        z = np.zeros_like(f); one = np.zeros_like(f); one[Cc // 3, 0, 0] = 2.5
        variants += [z, one]
    else:
        f[:, 0, 1] = 0                                         # the zero-norm pixel: N1 gives NaN, the rows give 0
        f[:, gh - 1, gw - 2] = 0; f[Cc - 1, gh - 1, gw - 2] = 0.125   # one non-zero channel: exactly 32767
    for v in variants:
        exp = sel.quantize(oracle, v)
        for dev in (False, True):
            got = ctx.feat_quantize(v, dev=dev)
            assert got.dtype == np.int16 and np.array_equal(got, exp), (Cc, grid, dev)
    if gh * gw == 1:
        assert not sel.quantize(oracle, variants[1]).any() and sel.quantize(oracle, variants[2])[0, Cc // 3] == 32767
    else:
        assert not exp[1].any() and exp[(gh - 1) * gw + gw - 2, Cc - 1] == 32767 and np.count_nonzero(exp[(gh - 1) * gw + gw - 2]) == 1


# ---------------------------------------------------------------- nct_region_score
def unit_rows(rng, n, Cc):
    """n int16 rows of norm 32767 up to rounding, as rule 2 makes them"""
    x = rng.standard_normal((n, Cc))
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    return np.rint(x * 32767).astype(np.int16)


SCORE_CASES = [(1, 64, 1, 0), (63, 64, 5, 1), (64, 512, 64, 0), (65, 64, 64, 1), (65, 512, 65, 65), (1000, 64, 300, 65), (1000, 512, 5, 0), (127, 64, 63, 1),
               (128, 64, 64, 65), (129, 512, 1, 65), (1000, 68, 65, 1), (63, 4, 5, 65)]


@pytest.mark.parametrize("case", SCORE_CASES)
def test_region_score(ctx, case):
    cells, Cc, n_in, n_out = case
    rng = np.random.default_rng(cells * 7 + Cc + n_in * 3 + n_out)
    q, si, so = unit_rows(rng, cells, Cc), unit_rows(rng, n_in, Cc), unit_rows(rng, n_out, Cc)
    # some queries are seeds of either class, so that the maxima are not all near zero
    q[:: 3] = si[rng.integers(0, n_in, len(q[:: 3]))]
    if n_out:
        q[1:: 5] = so[rng.integers(0, n_out, len(q[1:: 5]))]
    for sharp, fl in ((1024, 700), (1, 0), (65536, 1000), (37, 333)):
        exp = sel.score(q, si, so, sharp, fl)
        for dev in (False, True):
            got = ctx.region_score(q, si, so if n_out else None, sharp, fl, dev=dev)
            assert np.array_equal(got, exp), (case, sharp, fl, dev)


def test_region_score_adversarial(ctx):
    rng = np.random.default_rng(11)
    Cc = 64
    row = unit_rows(rng, 1, Cc)
    # all rows identical: d = 0 gives 128 at every sharpness; without outside seeds floor_permille decides
    q = np.repeat(row, 130, axis=0)
    for sharp in (1, 1024, 65536):
        got = ctx.region_score(q, np.repeat(row, 65, axis=0), np.repeat(row, 3, axis=0), sharp, 700)
        assert (got == 128).all() and np.array_equal(got, sel.score(q, q[:65], q[:3], sharp, 700))
    for fl in (0, 700, 999, 1000):
        got = ctx.region_score(q, q[:5], None, 1024, fl)
        assert np.array_equal(got, sel.score(q, q[:5], None, 1024, fl)), fl
    assert (ctx.region_score(q, q[:5], None, 1024, 0) == 255).all()
    # zero query rows: both maxima are 0
    z = np.zeros((70, Cc), np.int16)
    si, so = unit_rows(rng, 66, Cc), unit_rows(rng, 2, Cc)
    assert (ctx.region_score(z, si, so, 65536, 700) == 128).all()
    assert np.array_equal(ctx.region_score(z, si, None, 1024, 700), sel.score(z, si, None, 1024, 700)) and (ctx.region_score(z, si, None, 1024, 700) == 0).all()
    # rows with one component at +-32767: the dot product sits at +-32767^2 or at 0
    for Cc in (64, 512):
        e = np.zeros((2 * Cc, Cc), np.int16)
        e[np.arange(Cc), np.arange(Cc)] = 32767
        e[Cc + np.arange(Cc), np.arange(Cc)] = -32767
        si, so = e[[0, Cc + 1, Cc - 1]], e[[Cc, 1, 2 * Cc - 1]]
        for sharp in (1, 1024, 65536):
            exp = sel.score(e, si, so, sharp, 700)
            for dev in (False, True):
                assert np.array_equal(ctx.region_score(e, si, so, sharp, 700, dev=dev), exp), (Cc, sharp, dev)
        exp = sel.score(e, si, so, 1024, 700)
        assert exp.min() == 0 and exp.max() == 255 and (exp == 128).any()       # saturated at both ends, and the cells that meet no seed's component
        assert np.array_equal(ctx.region_score(e, si, None, 1, 1000), sel.score(e, si, None, 1, 1000))


def test_region_score_bench_hook(ctx):
    """the measurement hook runs the same kernel: its output is the rule's, its time positive, its refusals named"""
    rng = np.random.default_rng(3)
    q, si, so = unit_rows(rng, 300, 128), unit_rows(rng, 70, 128), unit_rows(rng, 9, 128)
    ms = C.c_float(-1)
    with ctx.blocks() as b:
        blocks = [b.up(q), b.up(si), b.up(so), b.new(300)]
        args = [blocks[0], 300, 128, blocks[1], 70, blocks[2], 9, 1024, 700, blocks[3]]
        ctx._chk(ctx._l.nct_region_score_bench(ctx._h, *args, 3, C.byref(ms)))
        assert ms.value > 0 and np.array_equal(ctx.dev_download(blocks[3], (300,), np.uint8), sel.score(q, si, so))
        raw_refused(ctx, "nct_region_score_bench", args + [0, C.byref(ms)], INVALID, "reps")
        raw_refused(ctx, "nct_region_score_bench", args + [1001, C.byref(ms)], INVALID, "reps")
        raw_refused(ctx, "nct_region_score_bench", args + [1, None], INVALID, "kernel_ms")


# ---------------------------------------------------------------- the whole call
CALLS = [(size, tap, iters, 7) for size in sel.SIZES for tap in (1, 2, 3, 5) for iters in (0, 1, 2)] + [(size, 5, 1, 1) for size in sel.SIZES]


@pytest.mark.parametrize("size,tap,iters,max_seeds", CALLS)
def test_region_select(wctx, oracle, weights, sources, size, tap, iters, max_seeds):
    src, taps = sources[size]
    T = sel.call_strokes(*size)
    exp, est = sel.select(oracle, src, T, *weights, tap=tap, max_seeds=max_seeds, snap_iters=iters, feat=taps[tap - 1])
    if tap <= 3 or max_seeds == 1:                             # both classes are subsampled
        assert (est["cell"] == sel.IN_DROPPED).any() and (est["cell"] == sel.OUT_DROPPED).any()
    p = nct.region_select_params(tap=tap, max_seeds=max_seeds, snap_iters=iters)
    got, st = wctx.region_select(src, T, p, want_stages=True)
    for k in ("q", "cell", "score", "up"):
        assert np.array_equal(st[k], est[k]), (k, size, tap, iters)
    assert np.array_equal(got, exp)
    assert np.array_equal(wctx.region_select(src, T, p), exp)
    assert np.array_equal(wctx.region_select(src, T, p, dev=True), exp)


@pytest.mark.parametrize("size", sel.SIZES)
def test_region_select_without_outside_strokes_and_defaults(wctx, oracle, weights, sources, size):
    src, taps = sources[size]
    T = sel.call_strokes(*size, outside=False)
    for fl in (700, 990):
        exp, est = sel.select(oracle, src, T, *weights, floor_permille=fl, feat=taps[1])
        got, st = wctx.region_select(src, T, nct.region_select_params(floor_permille=fl) if fl != 700 else None, want_stages=True)
        assert not np.isin(est["cell"], (sel.OUT_KEPT, sel.OUT_DROPPED, sel.MIXED)).any()
        for k in ("q", "cell", "score", "up"):
            assert np.array_equal(st[k], est[k]), (k, size, fl)
        assert np.array_equal(got, exp)
    assert np.array_equal(wctx.region_select(src, T, None, dev=True), sel.select(oracle, src, T, *weights, feat=taps[1])[0])
    # the other parameters reach the kernels: a sharpness and a snap of their own
    T = sel.call_strokes(*size)
    exp, _ = sel.select(oracle, src, T, *weights, tap=2, sharpness=9, snap_iters=1, snap=(2, 25, 0), feat=taps[1])
    assert np.array_equal(wctx.region_select(src, T, nct.region_select_params(sharpness=9, radius=2, sigma=25, binary=0)), exp)


def test_region_select_texture_fixture(wctx, oracle, weights):
    """the fixture of the CPU test through the library: the same bytes, so the same IoU"""
    img, T, obj = sel.texture_fixture()
    exp, _ = sel.select(oracle, img, T, *weights, snap_iters=0)
    got = wctx.region_select(img, T, nct.region_select_params(snap_iters=0))
    assert np.array_equal(got, exp) and sel.iou(got >= 128, obj) >= 0.90


# ---------------------------------------------------------------- compositions
def test_pair_select_region_equals_select_and_set(wctx):
    src, T = sel.call_source(H, W), sel.call_strokes(H, W)
    ref = synth.image(2000, 48, 60)
    p = nct.region_select_params(tap=2, max_seeds=7)
    wctx.pair_upload(src, ref)
    wctx.pair_select_region(T, p, protect=1)
    wctx.pair_run()
    a = wctx.pair_download()
    m = wctx.region_select(src, T, p)
    wctx.pair_upload(src, ref)
    wctx.pair_set_region(m, protect=1)
    wctx.pair_run()
    b = wctx.pair_download()
    assert np.array_equal(a, b)
    assert not np.array_equal(a, wctx.process_pair(src, ref)) and (a[m == 0] == src[m == 0]).all()


def test_seq_select_region_equals_select_and_set(wctx):
    """on the selected frame and on one tracked and snapped frame after it: both full frames, motion on"""
    frames, _ = rs.obj_frames(2, H, W, 4)
    ref = synth.image(2000, 48, 60)
    T = sel.call_strokes(H, W)
    p = nct.region_select_params(tap=2, max_seeds=7)

    def run(select_in_sequence):
        wctx.seq_begin(ref, (H, W, 3))
        try:
            wctx.seq_set_motion(*MOT)
            wctx.seq_set_region_tracking(True)
            wctx.seq_set_region_snap(True)
            if select_in_sequence:
                wctx.seq_select_region(frames[0], T, p)
            else:
                wctx.seq_set_region(wctx_matte)
            out = []
            for f in frames:
                r = wctx.seq_frame(f)
                out.append((r,) + wctx.seq_get_region())
            return out
        finally:
            wctx.seq_end()

    wctx_matte = wctx.region_select(frames[0], T, p)
    a, b = run(True), run(False)
    for t in range(2):
        assert np.array_equal(a[t][0], b[t][0]) and np.array_equal(a[t][1], b[t][1]) and a[t][2] == b[t][2] == t, t
    assert np.array_equal(a[0][1], wctx_matte) and not np.array_equal(a[1][1], wctx_matte)


def test_region_select_keeps_nothing(wctx, sources):
    src, _ = sources[(57, 67)]
    T = sel.call_strokes(57, 67)
    p = nct.region_select_params(tap=3, max_seeds=7, snap_iters=2)
    wctx.region_select(src, T, p)
    first = wctx.counter(nct.CTR_ARENA_BYTES)
    for dev in (False, True, False):
        wctx.region_select(src, T, p, dev=dev)
        assert wctx.counter(nct.CTR_ARENA_BYTES) == first


# ---------------------------------------------------------------- refusals
def test_region_select_refusals(wctx, sources):
    src, _ = sources[(H, W)]
    T = sel.call_strokes(H, W)
    # no inside seed: none marked; outside strokes only; an inside stroke that lies only in mixed cells
    only_out = np.where(T == sel.OUT, T, 0).astype(np.uint8)
    mixed = np.zeros((H, W), np.uint8); mixed[20, 20] = sel.IN; mixed[21, 21] = sel.OUT
    for strokes in (np.zeros((H, W), np.uint8), only_out, mixed):
        for dev in (False, True):
            refused(lambda: wctx.region_select(src, strokes, nct.region_select_params(tap=2), dev=dev), INVALID, "no inside seed")
    assert wctx.region_select(src, mixed, nct.region_select_params(tap=1)).shape == (H, W)        # at tap 1 the two pixels are two cells
    # each parameter just outside its range
    for kw in (dict(tap=0), dict(tap=6), dict(sharpness=0), dict(sharpness=65537), dict(floor_permille=-1), dict(floor_permille=1001), dict(max_seeds=0), dict(max_seeds=4097),
               dict(snap_iters=-1), dict(snap_iters=9), dict(radius=0), dict(radius=9), dict(sigma=0), dict(sigma=256), dict(binary=2), dict(binary=-1)):
        for dev in (False, True):
            refused(lambda: wctx.region_select(src, T, nct.region_select_params(**kw), dev=dev), INVALID, next(iter(kw)))
    # each parameter at the ends of its range is taken
    for kw in (dict(tap=5, sharpness=1, floor_permille=0, max_seeds=1, snap_iters=0), dict(tap=1, sharpness=65536, floor_permille=1000, max_seeds=4096, snap_iters=8, radius=1, sigma=255)):
        wctx.region_select(src, T, nct.region_select_params(**kw))
    # a side of 16 and of 4001
    for shape, word in (((16, 64), "h must"), ((4001, 17), "h must"), ((64, 16), "w must"), ((17, 4001), "w must")):
        img, st = np.zeros(shape + (3,), np.uint8), np.full(shape, sel.IN, np.uint8)
        for dev in (False, True):
            refused(lambda: wctx.region_select(img, st, None, dev=dev), INVALID, word)
    # null pointers
    out = np.zeros((H, W), np.uint8)
    a = (src.ctypes.data, H, W, T.ctypes.data, None, out.ctypes.data)
    for i, word in ((0, "src_bgr"), (3, "strokes"), (5, "mask_out")):
        args = list(a); args[i] = None
        raw_refused(wctx, "nct_region_select", args + [None], INVALID, word)
        raw_refused(wctx, "nct_region_select_dev", args, INVALID, word)
    f, q = np.zeros((64, 2, 2), np.float32), np.zeros((4, 64), np.int16)
    raw_refused(wctx, "nct_feat_quantize", [None, q.ctypes.data, 64, 2, 2], INVALID, "src_chw")
    raw_refused(wctx, "nct_feat_quantize", [f.ctypes.data, None, 64, 2, 2], INVALID, "dst")
    raw_refused(wctx, "nct_feat_quantize", [f.ctypes.data, q.ctypes.data, 66, 2, 2], INVALID, "C must")
    raw_refused(wctx, "nct_feat_quantize_dev", [None, q.ctypes.data, 64, 2, 2], INVALID, "d_src_hwc")
    s = (q.ctypes.data, 4, 64, q.ctypes.data, 2, q.ctypes.data, 2, 1024, 700, out.ctypes.data)
    for i, v, word in ((0, None, "null q"), (3, None, "seeds_in"), (5, None, "seeds_out"), (9, None, "score_out"), (1, 0, "cells"), (2, 66, "C must"), (4, 0, "n_in"), (6, -1, "n_out"),
                       (7, 0, "sharpness"), (7, 65537, "sharpness"), (8, -1, "floor_permille"), (8, 1001, "floor_permille")):
        args = list(s); args[i] = v
        raw_refused(wctx, "nct_region_score", args, INVALID, word)
        raw_refused(wctx, "nct_region_score_dev", args, INVALID, word)


def test_region_select_needs_weights_and_the_compositions_their_state(weights):
    src, T = sel.call_source(H, W), sel.call_strokes(H, W)
    ref = synth.image(2000, 48, 60)
    with nct.Context(0) as c:
        refused(lambda: c.region_select(src, T), STATE, "weights")
        refused(lambda: c.region_select(src, T, dev=True), STATE, "weights")
        rg = nct.RegionParams.default()
        raw_refused(c, "nct_pair_select_region", [T.ctypes.data, None, C.addressof(rg)], STATE, "no source")
        raw_refused(c, "nct_seq_select_region", [src.ctypes.data, T.ctypes.data, None, C.addressof(rg)], STATE, "no sequence")
        c.pair_upload(src, ref)
        refused(lambda: c.pair_select_region(T), STATE, "weights")
        c.vgg19_load_raw(*weights)
        refused(lambda: c.pair_select_region(T, protect=2), INVALID, "protect")
        refused(lambda: c.pair_select_region(T, nct.region_select_params(tap=6)), INVALID, "tap")
        refused(lambda: c.pair_select_region(np.zeros_like(T)), INVALID, "no inside seed")
        raw_refused(c, "nct_pair_select_region", [None, None, None], INVALID, "strokes")
        c.pair_select_region(T)
        # an open sequence: the pair form is refused; the sequence form takes a frame, and refuses a null one
        c.seq_begin(ref, (H, W, 3))
        raw_refused(c, "nct_pair_select_region", [T.ctypes.data, None, None], STATE, "sequence is open")
        raw_refused(c, "nct_seq_select_region", [None, T.ctypes.data, None, None], INVALID, "frame_bgr")
        raw_refused(c, "nct_seq_select_region", [src.ctypes.data, None, None, None], INVALID, "strokes")
        refused(lambda: c.seq_select_region(src, T, protect=3), INVALID, "protect")
        refused(lambda: c.seq_select_region(src, np.zeros_like(T)), INVALID, "no inside seed")
        refused(lambda: c.seq_get_region(), STATE, "no region mask")                     # a refused call sets nothing
        c.seq_select_region(src, T)
        assert c.seq_get_region()[1] == 0
        c.seq_end()
        # the full-resolution sequence
        big, bigT = sel.call_source(2 * H, 2 * W), np.full((2 * H, 2 * W), sel.IN, np.uint8)
        c.seq_begin_fullres(ref, big.shape, max_side=W)
        refused(lambda: c.seq_select_region(big, bigT), STATE, "full-resolution")
        c.seq_end()
