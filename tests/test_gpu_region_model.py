"""Region models (SPEC §6.17) on the GPU, byte for byte against the numpy rule (tests/region_model_ref.py): the re-find seam nct_region_refind[_dev] with its refusals,
the model calls (fit, add, rows, from_rows), nct_region_model_apply[_dev] with its stages, and the composition with the region setter of a pair.

The re-find kernel's edges (k_region_refind.hip), all hit by rm.REFIND_CASES: a workgroup owns a 32 x 8 tile of the target (one tile; 57 x 67 and 40 x 300: partial tiles
on both axes, ten tiles across); widths 64 and 300 take the four-pixels-per-thread form, 7, 4, 67 and 41 the byte form; 33 x 40 -> 34 x 41 stages the largest LDS
footprint per tile; equal sizes are the copy."""
import ctypes as C

import numpy as np
import pytest

import nct
import region_model_ref as rm
import region_ref
import region_select_ref as sel
import synth

pytestmark = pytest.mark.gpu

INVALID, STATE = -2, -5
H, W = 56, 64


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


def second_image(h, w):
    """the call source shifted by (3, 5) under new noise"""
    img = np.roll(sel.call_source(h, w), (3, 5), (0, 1)).astype(int)
    return np.ascontiguousarray(np.clip(img + np.random.default_rng(77).integers(-4, 5, img.shape), 0, 255).astype(np.uint8))


@pytest.fixture(scope="module")
def sources(oracle, weights):
    """per size of sel.SIZES: the source, the oracle's taps 1 to 3 of it, the second image and its taps, computed once"""
    out = {}
    for h, w in sel.SIZES:
        src, nxt = sel.call_source(h, w), second_image(h, w)
        out[(h, w)] = (src, oracle.vgg19_features(src, *weights, deepest_tap=3), nxt, oracle.vgg19_features(nxt, *weights, deepest_tap=3))
    return out


def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def raw_refused(c, fn, args, code, word):
    rc = getattr(c._l, fn)(c._h, *args)
    msg = c._l.nct_last_error(c._h).decode()
    assert rc == code and word in msg, (fn, rc, msg)


# ---------------------------------------------------------------- nct_region_refind
@pytest.mark.parametrize("case", rm.REFIND_CASES)
def test_region_refind(ctx, oracle, case):
    (ht, wt), (Ht, Wt) = case
    for kind in rm.SCORE_KINDS:
        for margin in rm.MARGINS:
            score, prior = rm.refind_inputs(case, kind, margin)
            r = region_ref.resize_u8c1(oracle, score, Ht, Wt)
            for pr in (prior, None):
                exp = rm.refind(oracle, score, (Ht, Wt), pr, margin)
                for dev in (False, True):
                    got = ctx.region_refind(score, (Ht, Wt), pr, margin, dev=dev)
                    assert got.dtype == np.uint8 and np.array_equal(got, exp), (case, kind, margin, pr is None, dev)
                if pr is None or margin == 0:
                    assert np.array_equal(exp, r) and np.array_equal(exp, ctx.resize_u8c1(score, Ht, Wt))
                elif margin == 128:
                    assert np.array_equal(exp, prior)


def test_region_refind_dev_unaligned_and_neighbours(ctx, oracle):
    """W % 4 == 0 with an output or a prior that is not dword aligned takes the byte form; either way the inputs and the bytes around the output stay as they were"""
    case = ((28, 32), (56, 64))
    score, prior = rm.refind_inputs(case, "random", 32)
    exp = rm.refind(oracle, score, (56, 64), prior, 32)
    n = 56 * 64
    for so, sp in ((0, 0), (1, 0), (0, 2), (3, 1), (4, 4)):
        with ctx.blocks() as b:
            blocks = [b.up(score), b.up(np.concatenate([np.zeros(sp, np.uint8), prior.ravel(), np.zeros(8, np.uint8)])), b.up(np.full(n + 16, 0x5a, np.uint8))]
            ctx._chk(ctx._l.nct_region_refind_dev(ctx._h, blocks[0], 28, 32, blocks[1] + sp, 56, 64, 32, blocks[2] + so))
            whole = ctx.dev_download(blocks[2], (n + 16,), np.uint8)
            assert np.array_equal(whole[so:so + n].reshape(56, 64), exp), (so, sp)
            assert (whole[:so] == 0x5a).all() and (whole[so + n:] == 0x5a).all(), (so, sp)
            assert np.array_equal(ctx.dev_download(blocks[0], (28, 32), np.uint8), score)
            assert np.array_equal(ctx.dev_download(blocks[1], (sp + n + 8,), np.uint8)[sp:sp + n].reshape(56, 64), prior)


def test_region_refind_bench_hook(ctx, oracle):
    """the measurement hook runs the same kernel: its output is the rule's, its time positive, its refusals named"""
    case = ((29, 34), (57, 67))
    score, prior = rm.refind_inputs(case, "random", 32)
    ms = C.c_float(-1)
    with ctx.blocks() as b:
        blocks = [b.up(score), b.up(prior), b.new(57 * 67)]
        args = [blocks[0], 29, 34, blocks[1], 57, 67, 32, blocks[2]]
        ctx._chk(ctx._l.nct_region_refind_bench(ctx._h, *args, 3, C.byref(ms)))
        assert ms.value > 0 and np.array_equal(ctx.dev_download(blocks[2], (57, 67), np.uint8), rm.refind(oracle, score, (57, 67), prior, 32))
        raw_refused(ctx, "nct_region_refind_bench", args + [0, C.byref(ms)], INVALID, "reps")
        raw_refused(ctx, "nct_region_refind_bench", args + [1001, C.byref(ms)], INVALID, "reps")
        raw_refused(ctx, "nct_region_refind_bench", args + [1, None], INVALID, "kernel_ms")


def test_region_refind_refusals(ctx):
    score, prior, out = np.zeros((4, 5), np.uint8), np.zeros((8, 9), np.uint8), np.zeros((8, 9), np.uint8)
    good = (score.ctypes.data, 4, 5, prior.ctypes.data, 8, 9, 32, out.ctypes.data)
    for i, v, word in ((0, None, "null score"), (7, None, "null out"), (1, 0, "ht must"), (1, 4097, "ht must"), (2, 0, "wt must"), (2, 4097, "wt must"), (4, 3, "H must"),
                       (4, 16385, "H must"), (5, 4, "W must"), (5, 16385, "W must"), (6, -1, "margin"), (6, 129, "margin")):
        args = list(good); args[i] = v
        raw_refused(ctx, "nct_region_refind", args, INVALID, word)
        raw_refused(ctx, "nct_region_refind_dev", args, INVALID, word)
    for Hb, Wb in ((16384, 4097), (4097, 16384)):              # each side in range, the product above 2^26
        args = list(good); args[4] = Hb; args[5] = Wb
        raw_refused(ctx, "nct_region_refind", args, INVALID, "H * W")
        raw_refused(ctx, "nct_region_refind_dev", args, INVALID, "H * W")
    # the device form refuses an out that overlaps an input
    s, p = np.zeros((8, 9), np.uint8), np.zeros((8, 9), np.uint8)
    refused(lambda: ctx.region_refind(s, (8, 9), p, 32, dev=True, alias="score"), INVALID, "overlap score")
    refused(lambda: ctx.region_refind(s, (8, 9), p, 32, dev=True, alias="prior"), INVALID, "overlap prior")
    # the ends of the ranges are taken
    assert ctx.region_refind(np.full((1, 1), 9, np.uint8), (1, 1), None, 0).tolist() == [[9]]
    assert ctx.region_refind(np.full((1, 1), 9, np.uint8), (1, 1), np.full((1, 1), 3, np.uint8), 128).tolist() == [[3]]


# ---------------------------------------------------------------- the model calls
@pytest.mark.parametrize("size", sel.SIZES)
@pytest.mark.parametrize("tap", [1, 2, 3])
@pytest.mark.parametrize("max_seeds", [7, 4096])
def test_region_model_fit(wctx, oracle, weights, sources, size, tap, max_seeds):
    """the model's rows are the rows of nct_region_select's stages.q at the cells with codes 1 and 2, in raster order"""
    src, taps, _, _ = sources[size]
    T = sel.call_strokes(*size)
    p = nct.region_select_params(tap=tap, max_seeds=max_seeds, snap_iters=0)
    _, st = wctx.region_select(src, T, p, want_stages=True)
    code = st["cell"].ravel()
    model = wctx.region_model_fit(src, T, p)
    ri, ro = model.rows()
    assert model.info() == (tap, sel.TAP_C[tap - 1], len(ri), len(ro))
    assert np.array_equal(ri, st["q"][code == sel.IN_KEPT]) and np.array_equal(ro, st["q"][code == sel.OUT_KEPT])
    etap, eri, ero = rm.fit(oracle, src, T, *weights, tap=tap, max_seeds=max_seeds, feat=taps[tap - 1])
    assert np.array_equal(ri, eri) and np.array_equal(ro, ero)
    if max_seeds == 7:
        assert len(ri) == 7 and len(ro) == 7
    # from_rows round-trips
    again = nct.RegionModel(tap, ri, ro)
    assert again.info() == model.info() and all(np.array_equal(a, b) for a, b in zip(again.rows(), model.rows()))


def test_region_model_add_appends_and_refuses(wctx, oracle, weights, sources):
    src, taps, nxt, ntaps = sources[(H, W)]
    T = sel.call_strokes(H, W)
    p = nct.region_select_params(tap=2, max_seeds=7)
    model = wctx.region_model_fit(src, T, p)
    first = model.rows()
    wctx.region_model_add(model, nxt, T, nct.region_select_params(tap=2, max_seeds=5))
    exp = rm.add(rm.fit(oracle, src, T, *weights, tap=2, max_seeds=7, feat=taps[1]), rm.fit(oracle, nxt, T, *weights, tap=2, max_seeds=5, feat=ntaps[1]))
    ri, ro = model.rows()
    assert model.info() == (2, 128, 12, 12) and np.array_equal(ri, exp[1]) and np.array_equal(ro, exp[2])
    assert np.array_equal(ri[:7], first[0]) and np.array_equal(ro[:7], first[1])
    # strokes without an outside class add inside rows only
    wctx.region_model_add(model, src, sel.call_strokes(H, W, outside=False), p)
    assert model.info() == (2, 128, 19, 12)
    kept = model.rows()
    # refusals leave the model as it was
    refused(lambda: wctx.region_model_add(model, src, T, nct.region_select_params(tap=3)), INVALID, "not the model's tap")
    refused(lambda: wctx.region_model_add(model, src, T, nct.region_select_params(tap=6)), INVALID, "tap must")
    refused(lambda: wctx.region_model_add(model, src, np.zeros_like(T), p), INVALID, "no inside seed")
    refused(lambda: wctx.region_model_add(model, src, T, nct.region_select_params(max_seeds=0)), INVALID, "max_seeds")
    raw_refused(wctx, "nct_region_model_add", [None, src.ctypes.data, H, W, T.ctypes.data, None], INVALID, "null model")
    raw_refused(wctx, "nct_region_model_add", [model._m, None, H, W, T.ctypes.data, None], INVALID, "src_bgr")
    raw_refused(wctx, "nct_region_model_add", [model._m, src.ctypes.data, H, W, None, None], INVALID, "strokes")
    assert model.info() == (2, 128, 19, 12) and all(np.array_equal(a, b) for a, b in zip(model.rows(), kept))
    # a class that would exceed 65536 rows
    full = nct.RegionModel(2, np.zeros((65530, 128), np.int16), np.zeros((3, 128), np.int16))
    refused(lambda: wctx.region_model_add(full, src, T, p), INVALID, "inside rows")
    assert full.info() == (2, 128, 65530, 3)
    full = nct.RegionModel(2, np.zeros((3, 128), np.int16), np.zeros((65530, 128), np.int16))
    refused(lambda: wctx.region_model_add(full, src, T, p), INVALID, "outside rows")
    assert full.info() == (2, 128, 3, 65530)
    wctx.region_model_add(full, src, T, nct.region_select_params(tap=2, max_seeds=6))          # exactly 65536 is taken
    assert full.info() == (2, 128, 9, 65536)


def test_region_model_fit_refusals(wctx, sources):
    src, _, _, _ = sources[(H, W)]
    T = sel.call_strokes(H, W)
    only_out = np.where(T == sel.OUT, T, 0).astype(np.uint8)
    refused(lambda: wctx.region_model_fit(src, only_out), INVALID, "no inside seed")
    for kw in (dict(tap=0), dict(tap=6), dict(max_seeds=0), dict(max_seeds=4097)):
        refused(lambda: wctx.region_model_fit(src, T, nct.region_select_params(**kw)), INVALID, next(iter(kw)))
    for shape, word in (((16, 64), "h must"), ((17, 4001), "w must")):
        refused(lambda: wctx.region_model_fit(np.zeros(shape + (3,), np.uint8), np.full(shape, sel.IN, np.uint8)), INVALID, word)
    m = C.c_void_p()
    raw_refused(wctx, "nct_region_model_fit", [None, H, W, T.ctypes.data, None, C.byref(m)], INVALID, "src_bgr")
    raw_refused(wctx, "nct_region_model_fit", [src.ctypes.data, H, W, None, None, C.byref(m)], INVALID, "strokes")
    raw_refused(wctx, "nct_region_model_fit", [src.ctypes.data, H, W, T.ctypes.data, None, None], INVALID, "null model")
    assert not m.value


# ---------------------------------------------------------------- nct_region_model_apply
APPLY = [(size, tap, iters, with_prior) for size in sel.SIZES for tap in (1, 2, 3) for iters in (0, 2) for with_prior in (False, True)]


@pytest.mark.parametrize("size,tap,iters,with_prior", APPLY)
def test_region_model_apply(wctx, oracle, weights, sources, size, tap, iters, with_prior):
    src, taps, nxt, ntaps = sources[size]
    T = sel.call_strokes(*size)
    emodel = rm.fit(oracle, src, T, *weights, tap=tap, max_seeds=7, feat=taps[tap - 1])
    model = wctx.region_model_fit(src, T, nct.region_select_params(tap=tap, max_seeds=7))
    # a prior that disagrees with the score in places: the selection's own matte of the first image, not shifted
    prior = sel.select(oracle, src, T, *weights, tap=tap, max_seeds=7, snap_iters=1, feat=taps[tap - 1])[0] if with_prior else None
    p = nct.region_refind_params(snap_iters=iters)
    exp, est = rm.apply(oracle, emodel, nxt, *weights, prior=prior, snap_iters=iters, feat=ntaps[tap - 1])
    got, st = wctx.region_model_apply(model, nxt, prior, p, want_stages=True)
    for k in ("q", "score", "refound"):
        assert np.array_equal(st[k], est[k]), (k, size, tap, iters, with_prior)
    assert np.array_equal(got, exp)
    assert np.array_equal(wctx.region_model_apply(model, nxt, prior, p), exp)
    assert np.array_equal(wctx.region_model_apply(model, nxt, prior, p, dev=True), exp)
    # stages.m is nct_region_score of stages.q and the model's rows
    ri, ro = model.rows()
    assert np.array_equal(st["score"].ravel(), wctx.region_score(st["q"], ri, ro))
    if with_prior:
        r = region_ref.resize_u8c1(oracle, est["score"], *size)
        assert ((est["refound"] == r) | (est["refound"] == prior)).all()
        assert not np.array_equal(est["refound"], r) and not np.array_equal(est["refound"], prior)     # both sources are taken somewhere


def test_region_model_apply_parameters_and_a_model_from_rows(wctx, oracle, weights, sources):
    src, taps, nxt, ntaps = sources[(57, 67)]
    T = sel.call_strokes(57, 67)
    emodel = rm.fit(oracle, src, T, *weights, tap=2, max_seeds=7, feat=taps[1])
    model = nct.RegionModel(*emodel)                            # built from the reference's rows
    prior = np.random.default_rng(5).integers(0, 256, (57, 67)).astype(np.uint8)
    for kw, ekw in ((dict(sharpness=9, margin=5), dict(sharpness=9, margin=5)), (dict(margin=0), dict(margin=0)), (dict(margin=128, snap_iters=0), dict(margin=128, snap_iters=0)),
                    (dict(radius=2, sigma=25, binary=0), dict(snap=(2, 25, 0))), (dict(floor_permille=990), dict(floor_permille=990))):
        exp, _ = rm.apply(oracle, emodel, nxt, *weights, prior=prior, feat=ntaps[1], **ekw)
        assert np.array_equal(wctx.region_model_apply(model, nxt, prior, nct.region_refind_params(**kw)), exp), kw
    assert np.array_equal(wctx.region_model_apply(model, nxt, prior, nct.region_refind_params(margin=128, snap_iters=0)), prior)
    # the defaults, and a model without outside rows: floor_permille decides
    exp, _ = rm.apply(oracle, emodel, nxt, *weights, feat=ntaps[1])
    assert np.array_equal(wctx.region_model_apply(model, nxt), exp)
    inside_only = (2, emodel[1], emodel[2][:0])
    exp, _ = rm.apply(oracle, inside_only, nxt, *weights, feat=ntaps[1])
    assert np.array_equal(wctx.region_model_apply(nct.RegionModel(2, emodel[1]), nxt), exp)


def test_region_model_apply_keeps_nothing(wctx, sources):
    src, _, nxt, _ = sources[(57, 67)]
    T = sel.call_strokes(57, 67)
    model = wctx.region_model_fit(src, T, nct.region_select_params(tap=3, max_seeds=7))
    p = nct.region_refind_params(snap_iters=2)
    prior = np.zeros((57, 67), np.uint8)
    wctx.region_model_apply(model, nxt, prior, p)
    first = wctx.counter(nct.CTR_ARENA_BYTES)
    for dev in (False, True, False):
        wctx.region_model_apply(model, nxt, prior, p, dev=dev)
        wctx.region_model_fit(src, T, nct.region_select_params(tap=3, max_seeds=7)).close()
        assert wctx.counter(nct.CTR_ARENA_BYTES) == first


def test_region_model_apply_refusals(wctx, weights, sources):
    src, _, nxt, _ = sources[(H, W)]
    T = sel.call_strokes(H, W)
    model = wctx.region_model_fit(src, T, nct.region_select_params(max_seeds=7))
    for kw in (dict(sharpness=0), dict(sharpness=65537), dict(floor_permille=-1), dict(floor_permille=1001), dict(margin=-1), dict(margin=129), dict(snap_iters=-1),
               dict(snap_iters=9), dict(radius=0), dict(radius=9), dict(sigma=0), dict(sigma=256), dict(binary=2)):
        for dev in (False, True):
            refused(lambda: wctx.region_model_apply(model, nxt, None, nct.region_refind_params(**kw), dev=dev), INVALID, next(iter(kw)))
    for kw in (dict(sharpness=1, floor_permille=0, margin=0, snap_iters=0), dict(sharpness=65536, floor_permille=1000, margin=128, snap_iters=8, radius=1, sigma=255)):
        wctx.region_model_apply(model, nxt, None, nct.region_refind_params(**kw))
    for shape, word in (((16, 64), "h must"), ((4001, 17), "h must"), ((64, 16), "w must"), ((17, 4001), "w must")):
        for dev in (False, True):
            refused(lambda: wctx.region_model_apply(model, np.zeros(shape + (3,), np.uint8), dev=dev), INVALID, word)
    out = np.zeros((H, W), np.uint8)
    a = (model._m, nxt.ctypes.data, H, W, None, None, out.ctypes.data)
    for i, word in ((0, "null model"), (1, "src_bgr"), (6, "mask_out")):
        args = list(a); args[i] = None
        raw_refused(wctx, "nct_region_model_apply", args + [None], INVALID, word)
        raw_refused(wctx, "nct_region_model_apply_dev", args, INVALID, word)
    # the device form refuses a mask_out that overlaps an input
    with wctx.blocks() as b:
        blocks = [b.up(nxt), b.up(out)]
        raw_refused(wctx, "nct_region_model_apply_dev", [model._m, blocks[0], H, W, blocks[1], None, blocks[1]], INVALID, "overlap prior")
        raw_refused(wctx, "nct_region_model_apply_dev", [model._m, blocks[0], H, W, None, None, blocks[0]], INVALID, "overlap src_bgr")
    ref = synth.image(2000, 48, 60)
    with nct.Context(0) as c:
        refused(lambda: c.region_model_apply(model, nxt), STATE, "weights")
        refused(lambda: c.region_model_apply(model, nxt, dev=True), STATE, "weights")
        refused(lambda: c.region_model_fit(src, T), STATE, "weights")
        raw_refused(c, "nct_pair_apply_region_model", [model._m, None, None], STATE, "no source")
        c.pair_upload(nxt, ref)
        refused(lambda: c.pair_apply_region_model(model), STATE, "weights")
        c.vgg19_load_raw(*weights)
        refused(lambda: c.pair_apply_region_model(model, protect=2), INVALID, "protect")
        refused(lambda: c.pair_apply_region_model(model, nct.region_refind_params(margin=129)), INVALID, "margin")
        raw_refused(c, "nct_pair_apply_region_model", [None, None, None], INVALID, "null model")
        c.pair_apply_region_model(model)
        c.seq_begin(ref, (H, W, 3))
        raw_refused(c, "nct_pair_apply_region_model", [model._m, None, None], STATE, "sequence is open")
        c.seq_end()


# ---------------------------------------------------------------- the composition with a pair
def test_pair_apply_region_model_equals_apply_and_process_pair_region(wctx, sources):
    src, _, nxt, _ = sources[(H, W)]
    T = sel.call_strokes(H, W)
    ref = synth.image(2000, 48, 60)
    model = wctx.region_model_fit(src, T, nct.region_select_params(tap=2, max_seeds=7))
    p = nct.region_refind_params(snap_iters=1)
    wctx.pair_upload(nxt, ref)
    wctx.pair_apply_region_model(model, p, protect=1)
    wctx.pair_run()
    a = wctx.pair_download()
    m = wctx.region_model_apply(model, nxt, None, p)
    b = wctx.process_pair_region(nxt, m, ref, protect=1)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, wctx.process_pair(nxt, ref)) and (a[m == 0] == nxt[m == 0]).all() and (m == 0).any() and (m == 255).any()


# ---------------------------------------------------------------- sequences (rules S1 to S6)
import region_snap_ref as rs        # noqa: E402
import seq_auto_ref as ar           # noqa: E402
import seq_mc_ref                   # noqa: E402
import seq_track_ref as tr          # noqa: E402

REF = (2000, 48, 60)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
SNAP = (rs.RADIUS, rs.SIGMA, rs.BINARY)
LEVELS = 3
KINDS = "FPFP"


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _params(levels=LEVELS):
    p = nct.Params.default()
    p.levels = levels
    return p


@pytest.fixture(scope="module")
def ref():
    return synth.image(*REF)


@pytest.fixture(scope="module")
def clips():
    """per size of sel.SIZES: four frames of the object clip, 4 px per frame"""
    return {size: rs.obj_frames(4, *size, 4)[0] for size in sel.SIZES}


def run_clip(c, ref, frames, kinds, model=None, params=None, seq_snap=None, given=None, tracking=True, protect=None):
    """a working-size sequence, motion on: the model (None: none) is set before the first frame, given[t] (None: none) by nct_seq_set_region before frame t
    -> [(result, maps, the matte in force or None, its age)]"""
    c.seq_begin(ref, frames[0].shape, _params())
    try:
        c.seq_set_motion(*MOT)
        if tracking:
            c.seq_set_region_tracking(True)
        if seq_snap is not None:
            c.seq_set_region_snap(True, *seq_snap)
        if model is not None:
            c.seq_set_region_model(model, params, protect)
        got, have = [], False
        for t, (f, k) in enumerate(zip(frames, kinds)):
            if given is not None and given[t] is not None:
                c.seq_set_region(given[t], protect)
                have = True
            out, lv = c.seq_frame_propagate_levels(f) if k == "P" else c.seq_frame_levels(f, want_color=False)
            have = have or (model is not None and k != "P")
            m, age = c.seq_get_region() if have else (None, None)
            got.append((out, lv, m, age))
        return got
    finally:
        c.seq_end()


@pytest.mark.parametrize("size", sel.SIZES)
@pytest.mark.parametrize("seq_snap", [None, SNAP])
def test_seq_region_model_manual(wctx, oracle, weights, ref, clips, size, seq_snap):
    """F P F P with motion and tracking on, the model set before the first frame and no matte: the first frame gets one. After every frame the matte is the
    reference chain's — carry -> snap -> re-find on full frames, the carry (and the snap) alone on propagated ones, the fields read from nct_seq_levels.motion — and the
    bytes and the kept X' are those of a sequence without a model that is given those mattes"""
    frames = clips[size]
    T = sel.call_strokes(*size)
    sp = nct.region_select_params(tap=2, max_seeds=7)
    model = wctx.region_model_fit(frames[0], T, sp)
    emodel = rm.fit(oracle, frames[0], T, *weights, tap=2, max_seeds=7)
    assert all(np.array_equal(a, b) for a, b in zip(model.rows(), emodel[1:]))
    got = run_clip(wctx, ref, frames, KINDS, model, nct.region_refind_params(snap_iters=1), seq_snap)
    fields = [None] + [g[1]["motion"][LEVELS - 1] for g in got[1:]]
    assert any(f.any() for f in fields[1:])                                            # the pan is found
    M = rm.sequence_mattes(oracle, emodel, *weights, frames, KINDS, fields, seq_snap, snap_iters=1)
    for t, (out, lv, m, age) in enumerate(got):
        assert np.array_equal(m, M[t]), ("matte", t, int((m != M[t]).sum()))
        assert age == t, ("age", t)
    # frame 2 re-finds with a prior that matters: without it (or with the carry alone) the matte is another one
    carried = tr.matte_warp(M[1], fields[2])
    assert not np.array_equal(M[2], carried)
    assert np.array_equal(M[0], wctx.region_model_apply(model, frames[0], None, nct.region_refind_params(snap_iters=1)))
    manual = run_clip(wctx, ref, frames, KINDS, given=M, tracking=False)
    for t in range(4):
        assert np.array_equal(got[t][0], manual[t][0]), ("bytes", t)
        assert np.array_equal(manual[t][2], M[t])
        for l in range(LEVELS):
            assert np.array_equal(words(got[t][1]["ab_blend"][l]), words(manual[t][1]["ab_blend"][l])), ("kept X'", t, l)
    assert not np.array_equal(got[0][0], run_clip(wctx, ref, frames[:1], "F")[0][0])    # the matte acts


def test_seq_region_model_fresh_matte_and_other_taps(wctx, oracle, weights, ref, clips):
    """rule S1: a fresh matte's own frame uses it as it came, also with a model set; the next full frame re-finds with its carry as the prior. Taps 1 and 5 (conv5_1
    is the forward's own output), protect, snap_iters 0 and 2"""
    frames = clips[(H, W)]
    T = sel.call_strokes(H, W)
    m0 = tr.rect(H, W, 14, 42, 8, 40)
    for tap, iters, protect in ((1, 0, 1), (5, 2, 0)):
        model = wctx.region_model_fit(frames[0], T, nct.region_select_params(tap=tap, max_seeds=7))
        emodel = rm.fit(oracle, frames[0], T, *weights, tap=tap, max_seeds=7)
        given = [m0, None, None, None]
        p = nct.region_refind_params(snap_iters=iters, margin=48)
        got = run_clip(wctx, ref, frames, "FFPF", model, p, SNAP, given=given, protect=protect)
        assert np.array_equal(got[0][2], m0) and got[0][3] == 0
        fields = [None] + [g[1]["motion"][LEVELS - 1] for g in got[1:]]
        M = rm.sequence_mattes(oracle, emodel, *weights, frames, "FFPF", fields, SNAP, given=given, snap_iters=iters, margin=48)
        for t in range(4):
            assert np.array_equal(got[t][2], M[t]) and got[t][3] == t, ("matte", tap, t)
        manual = run_clip(wctx, ref, frames, "FFPF", given=M, tracking=False, protect=protect)
        for t in range(4):
            assert np.array_equal(got[t][0], manual[t][0]), ("bytes", tap, t)


def test_seq_region_model_auto_with_a_cut(wctx, oracle, weights, ref):
    """nct_seq_frame_auto on the cut clip (F P C P): the decisions are those without a model; the CUT frame's matte is nct_region_model_apply's with no prior; every
    frame's bytes are those of the manual calls the decisions name, each given the matte (the fields come from the CPU chain)"""
    fr, mot, auto = ar.clips(H, W)["cut"]
    au = nct.seq_auto(*auto)
    T = sel.call_strokes(H, W)
    model = wctx.region_model_fit(fr[0], T, nct.region_select_params(tap=2, max_seeds=7))
    emodel = rm.fit(oracle, fr[0], T, *weights, tap=2, max_seeds=7)
    p = nct.region_refind_params(snap_iters=1)
    strip = lambda d: {k: v for k, v in d.items() if k != "probe_ms"}
    wctx.seq_begin(ref, (H, W, 3), _params())
    try:
        wctx.seq_set_motion(*mot)
        plain_ds = [strip(wctx.seq_frame_auto(f, au)[1]) for f in fr]
    finally:
        wctx.seq_end()
    kinds = ar.kinds(plain_ds)
    assert kinds == "FPCP"
    labs = [tr.labs(oracle, f, LEVELS) for f in fr]
    fields = [None] + [tr.top_field(labs[t], labs[t - 1], mot) for t in range(1, 4)]
    M = rm.sequence_mattes(oracle, emodel, *weights, fr, kinds, fields, SNAP, zero_at=(2,), snap_iters=1)
    wctx.seq_begin(ref, (H, W, 3), _params())
    try:
        wctx.seq_set_motion(*mot)
        wctx.seq_set_region_tracking(True)
        wctx.seq_set_region_snap(True, *SNAP)
        wctx.seq_set_region_model(model, p)
        outs = []
        for t, f in enumerate(fr):
            if t > 0:
                assert strip(wctx.seq_probe(f, au)) == plain_ds[t], ("probe", t)
            o, d = wctx.seq_frame_auto(f, au)
            assert strip(d) == plain_ds[t], t
            got, age = wctx.seq_get_region()
            assert np.array_equal(got, M[t]) and age == t, ("matte", t)
            outs.append(o)
        # the same frames by hand, without a model
        wctx.seq_set_region_model(None)
        wctx.seq_reset()
        wctx.seq_set_region_tracking(False)
        for t, f in enumerate(fr):
            wctx.seq_set_region(M[t])
            if kinds[t] == "C":
                wctx.seq_reset()
            manual = wctx.seq_frame_propagate(f) if kinds[t] == "P" else wctx.seq_frame(f)
            assert np.array_equal(outs[t], manual), t
    finally:
        wctx.seq_end()
    assert np.array_equal(M[2], wctx.region_model_apply(model, fr[2], None, p))
    assert not np.array_equal(M[2], wctx.region_model_apply(model, fr[2], tr.matte_warp(M[1], fields[2]), p))        # the old shot's matte would have been taken in places


H0, W0, MAX_SIDE = 114, 134, 67


def test_seq_region_model_fullres(wctx, oracle, weights):
    """a full-resolution sequence with the upsampling finish, 114 x 134 originals at max_side 67 (working size 57 x 67): the original-size matte is the reference's
    direct re-find from the working-size tap grid, snapped with the original frame as the guide; the bytes are those of the sequence that is given those mattes"""
    f0, _ = rs.obj_frames(3, H0, W0, 8)                        # 4 px per frame at the working size
    ref0 = synth.image(2000, 100, 120)
    S = [oracle.resize_u8c3(f, 57, 67) for f in f0]
    T = sel.call_strokes(57, 67)
    model = wctx.region_model_fit(S[0], T, nct.region_select_params(tap=2, max_seeds=7))
    emodel = rm.fit(oracle, S[0], T, *weights, tap=2, max_seeds=7)
    p = nct.region_refind_params(snap_iters=1)
    kinds = "FPF"

    def run(with_model, given=None):
        wctx.seq_begin_fullres(ref0, f0[0].shape, MAX_SIDE, nct.FINISH_UPSAMPLE, _params())
        try:
            wctx.seq_set_motion(*MOT)
            if with_model:
                wctx.seq_set_region_tracking(True)
                wctx.seq_set_region_model(model, p)
            got = []
            for t, k in enumerate(kinds):
                if given is not None:
                    wctx.seq_set_region(given[t])
                out, lv = wctx.seq_frame_propagate_levels(f0[t]) if k == "P" else wctx.seq_frame_levels(f0[t])
                got.append((out, lv) + wctx.seq_get_region())
            return got
        finally:
            wctx.seq_end()

    got = run(True)
    fields = [None] + [g[1]["motion"][LEVELS - 1] for g in got[1:]]
    M = rm.sequence_mattes(oracle, emodel, *weights, S, kinds, fields, None, guides=f0, snap_iters=1)
    for t in range(3):
        assert got[t][2].shape == (H0, W0) and np.array_equal(got[t][2], M[t]) and got[t][3] == t, ("matte", t)
    # straight to the original size: not the working-size matte enlarged
    small, _ = rm.apply(oracle, emodel, S[0], *weights, snap_iters=0)
    direct, _ = rm.apply(oracle, emodel, S[0], *weights, snap_iters=0, guide=f0[0])
    assert not np.array_equal(direct, region_ref.resize_u8c1(oracle, small, H0, W0))
    manual = run(False, given=M)
    for t in range(3):
        assert np.array_equal(got[t][0], manual[t][0]), ("bytes", t)
        for l in range(LEVELS):
            assert np.array_equal(words(got[t][1]["ab_blend"][l]), words(manual[t][1]["ab_blend"][l])), ("kept X'", t, l)


def test_seq_without_a_model_is_the_sequence_of_before(wctx, oracle, weights, ref, clips):
    """never set, or set and removed before the first frame: the tracked and snapped sequence of the existing reference, byte for byte"""
    frames = clips[(H, W)]
    mattes = [tr.rect(H, W, 14, 42, 8, 40), None, None, None]
    kinds = "FBPB"
    exp, keeps, _, M, ages = rs.sequence(oracle, frames, mattes, ref, *weights, SNAP, kinds=kinds, mot=MOT, levels=LEVELS)
    model = wctx.region_model_fit(frames[0], sel.call_strokes(H, W), nct.region_select_params(max_seeds=7))
    for removed in (False, True):
        wctx.seq_begin(ref, (H, W, 3), _params())
        try:
            wctx.seq_set_motion(*MOT)
            wctx.seq_set_region_tracking(True)
            wctx.seq_set_region_snap(True, *SNAP)
            if removed:
                wctx.seq_set_region_model(model)
                wctx.seq_set_region_model(None)
            wctx.seq_set_region(mattes[0])
            for t, k in enumerate(kinds):
                out, lv = wctx.seq_frame_propagate_levels(frames[t]) if k == "P" else wctx.seq_frame_levels(frames[t], want_color=False)
                m, age = wctx.seq_get_region()
                assert np.array_equal(m, M[t]) and age == ages[t], ("matte", removed, t)
                assert np.array_equal(out, exp[t]), (removed, t)
                for l in range(LEVELS):
                    assert np.array_equal(words(lv["ab_blend"][l]), words(keeps[t]["ab_blend"][l])), ("kept X'", removed, t, l)
        finally:
            wctx.seq_end()


def test_seq_set_region_model_refusals_and_replacement(wctx, ref, clips):
    frames = clips[(H, W)]
    T = sel.call_strokes(H, W)
    model = wctx.region_model_fit(frames[0], T, nct.region_select_params(tap=2, max_seeds=7))
    other = wctx.region_model_fit(frames[0], T, nct.region_select_params(tap=3, max_seeds=3))
    refused(lambda: wctx.seq_set_region_model(model), STATE, "no sequence is open")
    refused(lambda: wctx.seq_set_region_model(None), STATE, "no sequence is open")
    p = nct.region_refind_params(snap_iters=0, margin=20)
    want = run_clip(wctx, ref, frames[:2], "FF", model, p)
    wctx.seq_begin(ref, (H, W, 3), _params())
    try:
        wctx.seq_set_motion(*MOT)
        wctx.seq_set_region_tracking(True)
        refused(lambda: wctx.seq_get_region(), STATE, "no region mask")
        wctx.seq_set_region_model(other)
        wctx.seq_set_region_model(model, p)                     # replaces it
        for kw in (dict(sharpness=0), dict(floor_permille=1001), dict(margin=129), dict(snap_iters=9), dict(radius=0), dict(sigma=256), dict(binary=2)):
            refused(lambda: wctx.seq_set_region_model(other, nct.region_refind_params(**kw)), INVALID, next(iter(kw)))
        refused(lambda: wctx.seq_set_region_model(other, None, protect=2), INVALID, "protect")
        refused(lambda: wctx.seq_get_region(), STATE, "no region mask")                  # a model alone is no matte yet
        for t in range(2):                                      # a refused call leaves the setting as it was
            out = wctx.seq_frame(frames[t])
            m, age = wctx.seq_get_region()
            assert np.array_equal(out, want[t][0]) and np.array_equal(m, want[t][2]) and age == want[t][3] == t, t
        # removed: the matte stays and is carried as before, full frames no longer re-find
        wctx.seq_set_region_model(None)
        before, _ = wctx.seq_get_region()
        wctx.seq_frame(frames[2])
        after, age = wctx.seq_get_region()
        lv = None
        assert age == 2 and not np.array_equal(after, before)
    finally:
        wctx.seq_end()
    assert not np.array_equal(want[1][2], want[0][2])
