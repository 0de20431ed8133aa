"""Motion-compensated frame sequences (SPEC §6.4) on the GPU: k_seq_motion and the blend through a field against the numpy rule (tests/seq_mc_ref.py), whole sequences
against the composition level by level, the identities of rule 6, what a context holds, the refusals, and the console driver's -motion 1. All comparisons are
equality of bytes / bit patterns."""
import os
import subprocess
import numpy as np
import pytest
from PIL import Image

import nct
import seq_mc_ref
import seq_ref
import synth

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "neural-color-transfer_amd", "bin", "neural_color_transfer")


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- seams: nct_seq_motion_field / nct_seq_blend_mc and their _dev forms against the numpy rule

def _check_motion(ctx, L, Lp, parent, R, penalty):
    exp = seq_mc_ref.motion(L, Lp, parent, R, penalty)
    got = ctx.seq_motion_field(L, Lp, parent, R, penalty)
    assert got.dtype == np.int16 and np.array_equal(got, exp)
    assert np.array_equal(ctx.seq_motion_field_dev(L, Lp, parent, R, penalty), exp)
    return exp


@pytest.mark.parametrize("grid,kind,with_parent,R,penalty", seq_mc_ref.MOTION_CASES)
def test_motion_field_matches_the_numpy_rule(ctx, grid, kind, with_parent, R, penalty):
    h, w = grid
    L, Lp, parent = seq_mc_ref.motion_case(h, w, 31 * h + w, kind, (seq_mc_ref.half(h), seq_mc_ref.half(w)) if with_parent else None)
    m = _check_motion(ctx, L, Lp, parent, R, penalty)
    if kind in ("equal", "flat") and not with_parent:
        assert not m.any()


def test_motion_field_from_level_to_level(ctx):
    """44 x 44 -> 88 x 88: the coarse field found at radius 3 is the parent of the fine search at radius 1; and 175 x 233 with a parent at radius 3"""
    fine, fine_p, _ = seq_mc_ref.motion_case(88, 88, 3, "random")
    coarse, coarse_p = fine[::2, ::2].copy(), fine_p[::2, ::2].copy()
    m0 = _check_motion(ctx, coarse, coarse_p, None, 3, 1)
    m1 = _check_motion(ctx, fine, fine_p, m0, 1, 1)
    assert m1.any()
    L, Lp, parent = seq_mc_ref.motion_case(175, 233, 9, "random", (88, 117))
    _check_motion(ctx, L, Lp, parent, 3, 1)
    L, Lp, _ = seq_mc_ref.motion_case(175, 233, 10, "noise")
    _check_motion(ctx, L, Lp, None, 8, 0)


def test_motion_field_on_a_700_level(ctx):
    """one 350 -> 700 level at the defaults' refinement radius; the maps are a smooth image under a shift of (1, -2), so the search has a field to find"""
    base = synth.image(1000, 704, 704)
    L = base[2:702, 2:702].copy(); Lp = base[1:701, 4:704].copy()               # L(q) = Lp(q + (1, -2))
    parent = np.zeros((350, 350, 2), np.int16); parent[..., 1] = -1
    m = _check_motion(ctx, L, Lp, parent, 1, 1)
    inner = m[8:-8, 8:-8]
    share = float(((inner[..., 0] == 1) & (inner[..., 1] == -2)).mean())
    print("700 level: share of inner pixels at (1, -2): %.4f" % share)
    assert share == 1.0                                                           # there the 25 taps match exactly: cost 0, and the comparison is strict


def _check_blend_mc(ctx, x, xp, lab, labp, tau, sigma, field):
    exp, etm = seq_mc_ref.blend_mc(x, xp, lab, labp, tau, sigma, field)
    got, tm = ctx.seq_blend_mc(x, xp, lab, labp, tau, sigma, field)
    assert np.array_equal(bits(tm), bits(etm)) and np.array_equal(bits(got), bits(exp))
    dev, dtm = ctx.seq_blend_mc_dev(x, xp, lab, labp, tau, sigma, field)
    assert np.array_equal(bits(dtm), bits(etm)) and np.array_equal(bits(dev), bits(exp))
    only, none = ctx.seq_blend_mc(x, xp, lab, labp, tau, sigma, field, want_tau_map=False)
    assert none is None and np.array_equal(bits(only), bits(exp))


@pytest.mark.parametrize("grid,kind", seq_ref.BLEND_CASES + [((9, 9), "nan_both"), ((11, 9), "random"), ((44, 44), "random"), ((88, 88), "nan_prev"), ((175, 233), "nan_both")])
@pytest.mark.parametrize("tau,sigma", [(0.7, 10.0), (0.85, 0.75)])
def test_blend_mc_matches_the_numpy_rule(ctx, grid, kind, tau, sigma):
    h, w = grid
    x, xp, lab, labp = seq_ref.blend_case(h, w, 17 * h + w, kind)
    rng = np.random.default_rng(h * 100 + w)
    _check_blend_mc(ctx, x, xp, lab, labp, tau, sigma, rng.integers(-3, 4, (h, w, 2)).astype(np.int16))
    _check_blend_mc(ctx, x, xp, lab, labp, tau, sigma, seq_mc_ref.motion(lab, labp, None, 3, 1))
    # without a field, and with an all-zero one, it is the plain blend
    exp, etm = seq_ref.blend(x, xp, lab, labp, tau, sigma)
    for field in (None, np.zeros((h, w, 2), np.int16)):
        got, tm = ctx.seq_blend_mc(x, xp, lab, labp, tau, sigma, field)
        assert np.array_equal(bits(tm), bits(etm)) and np.array_equal(bits(got), bits(exp))
    got, tm = ctx.seq_blend_mc_dev(x, xp, lab, labp, tau, sigma, None, alias_prev=True)       # NULL field: in place into x_prev is nct_seq_blend_dev's
    assert np.array_equal(bits(tm), bits(etm)) and np.array_equal(bits(got), bits(exp))


def test_blend_mc_on_a_700_level(ctx):
    x, xp, lab, labp = seq_ref.blend_case(700, 700, 7)
    field = np.random.default_rng(8).integers(-4, 5, (700, 700, 2)).astype(np.int16)
    _check_blend_mc(ctx, x, xp, lab, labp, 0.7, 10.0, field)


# ---- whole sequences against the composition

SRC, REF = (1000, 64, 56), (1001, 48, 64)


@pytest.mark.parametrize("levels,step", [(5, 2), (5, 4), (1, 2), (1, 4)])
def test_sequence_matches_the_composition_level_by_level(wctx, oracle, weights, levels, step):
    ws, bs = weights
    ref = synth.image(*REF)
    frames = seq_ref.pan_frames(3, SRC[1], SRC[2], step=step)
    exp, keeps = seq_mc_ref.sequence(oracle, frames, ref, ws, bs, levels=levels)
    # conditions on the expected side: the first frame has no field; with five levels the later frames carry one that is not zero at the finest level (with one level the
    # only grid is the coarsest, 4 x 4, where this pan is no motion)
    assert not any(m.any() for m in keeps[0]["motion"])
    assert levels == 1 or all(k["motion"][4].any() for k in keeps[1:])
    prm = nct.Params.default(); prm.levels = levels
    wctx.seq_begin(ref, frames[0].shape, prm)
    try:
        wctx.seq_set_motion()
        for t, f in enumerate(frames):
            out, lv = wctx.seq_frame_levels(f)
            for l in range(levels):
                assert np.array_equal(lv["motion"][l], keeps[t]["motion"][l]), ("motion", t, l)
                assert np.array_equal(bits(lv["color"][l]["ab_nonlocal"]), bits(keeps[t]["ab_nonlocal"][l])), ("ab_nonlocal", t, l)
                assert np.array_equal(bits(lv["tau_map"][l]), bits(keeps[t]["tau_map"][l])), ("tau_map", t, l)
                assert np.array_equal(bits(lv["ab_blend"][l]), bits(keeps[t]["ab_blend"][l])), ("ab_blend", t, l)
                assert np.array_equal(lv["result"][l], keeps[t]["result"][l]), ("result", t, l)
            assert np.array_equal(out, exp[t]), t
    finally:
        wctx.seq_end()
    # the plain entry point gives the same frames; motion set after the first frame takes effect from the next one
    wctx.seq_begin(ref, frames[0].shape, prm)
    try:
        assert np.array_equal(wctx.seq_frame(frames[0]), exp[0])
        wctx.seq_set_motion(3, 1, 1)
        for t in (1, 2):
            assert np.array_equal(wctx.seq_frame(frames[t]), exp[t]), t
    finally:
        wctx.seq_end()


# ---- identities (rule 6)

def test_motion_off_is_the_plain_sequence(wctx, weights):
    src, ref = synth.image(*SRC), synth.image(*REF)
    frames = seq_ref.pan_frames(3, SRC[1], SRC[2], step=2)
    try:
        wctx.seq_begin(ref, src.shape)
        plain = [wctx.seq_frame(f) for f in frames]
        wctx.seq_begin(ref, src.shape)
        wctx.seq_set_motion(0, 0, 5)                                                         # radii 0
        assert all(np.array_equal(wctx.seq_frame(f), p) for f, p in zip(frames, plain))
        wctx.seq_begin(ref, src.shape)
        wctx.seq_set_motion(off=True)                                                        # NULL
        out, lv = wctx.seq_frame_levels(frames[0])
        assert np.array_equal(out, plain[0])
        out, lv = wctx.seq_frame_levels(frames[1])
        assert np.array_equal(out, plain[1]) and not any(m.any() for m in lv["motion"])      # a frame without motion reports zeros
        # on, a frame, off again: the sequence goes on as a plain one from the state the motion frame left
        wctx.seq_begin(ref, src.shape)
        wctx.seq_set_motion()
        a0, a1 = wctx.seq_frame(frames[0]), wctx.seq_frame(frames[1])
        assert np.array_equal(a0, plain[0]) and not np.array_equal(a1, plain[1])
        wctx.seq_set_motion(off=True)
        a2 = wctx.seq_frame(frames[2])
        wctx.seq_begin(ref, src.shape)
        wctx.seq_set_motion()
        wctx.seq_frame(frames[0]); wctx.seq_frame(frames[1])
        wctx.seq_set_motion(0, 0, 1)                                                         # off by radii 0 is off by NULL
        assert np.array_equal(wctx.seq_frame(frames[2]), a2)
    finally:
        wctx.seq_end()
    with nct.Context(0) as c:                                                                # what a motion-off sequence holds
        c.vgg19_load_raw(*weights)
        c.seq_begin(ref, src.shape)
        c.seq_frame(frames[0])
        never = c.counter(nct.CTR_ARENA_BYTES)
        c.seq_end()
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        c.seq_begin(ref, src.shape)
        c.seq_set_motion(0, 0, 1)
        c.seq_set_motion(off=True)
        c.seq_frame(frames[0])
        print("arena bytes of an open sequence: never asked %d, motion off %d" % (never, c.counter(nct.CTR_ARENA_BYTES)))
        assert c.counter(nct.CTR_ARENA_BYTES) == never
        c.seq_set_motion()
        c.seq_frame(frames[1])
        assert c.counter(nct.CTR_ARENA_BYTES) > never                                        # the packed maps and the fields exist only while motion is on
        c.seq_end()


def test_identical_frames_two_contexts_and_reset(wctx, weights):
    src, ref = synth.image(*SRC), synth.image(*REF)
    frames = seq_ref.pan_frames(3, SRC[1], SRC[2], step=4)
    pair = wctx.process_pair(src, ref)
    try:
        for mot in ((3, 1, 1), (8, 3, 0)):
            wctx.seq_begin(ref, src.shape, tau=0.9, sigma=3.0)
            wctx.seq_set_motion(*mot)
            same = [wctx.seq_frame(src)] + [wctx.seq_frame_levels(src) for _ in range(2)]
            assert np.array_equal(same[0], pair)
            for out, lv in same[1:]:                                                         # (b): m = 0 and frame 0's output
                assert np.array_equal(out, pair) and not any(m.any() for m in lv["motion"])
        wctx.seq_begin(ref, src.shape)
        wctx.seq_set_motion()
        a = [wctx.seq_frame(f) for f in frames]
        wctx.seq_reset()                                                                     # the first frame after a reset is a pair; motion stays on
        assert np.array_equal(wctx.seq_frame(frames[2]), wctx_pair(wctx, frames[2], ref))
    finally:
        wctx.seq_end()
    with nct.Context(0) as c:                                                                # (d) the same sequence on another context
        c.vgg19_load_raw(*weights)
        c.seq_begin(ref, src.shape)
        c.seq_set_motion()
        b = [c.seq_frame(f) for f in frames]
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        c.seq_reset()
        again = [c.seq_frame(f) for f in frames]                                             # and twice on one context
        assert all(np.array_equal(x, y) for x, y in zip(a, again))


def wctx_pair(c, src, ref):
    """nct_process_pair of (src, ref) on a context of its own: the context under test has a sequence open"""
    with nct.Context(0) as p:
        from caffemodel_io import synthetic_vgg19
        p.vgg19_load_raw(*synthetic_vgg19(19))
        return p.process_pair(src, ref)


def test_pair_is_unchanged_after_a_motion_sequence(weights):
    src, ref = synth.image(*SRC), synth.image(*REF)
    frames = seq_ref.pan_frames(2, SRC[1], SRC[2], step=2)
    with nct.Context(0) as c:
        c.vgg19_load_raw(*weights)
        before = c.process_pair(src, ref)
        c.seq_begin(ref, src.shape)
        c.seq_set_motion()
        for f in frames:
            c.seq_frame(f)
        c.seq_end()
        assert np.array_equal(c.process_pair(src, ref), before)
        after = c.counter(nct.CTR_ARENA_BYTES)
        for _ in range(2):                                                                   # sequences with motion and pairs in turn: the arena stops growing
            c.seq_begin(ref, src.shape)
            c.seq_set_motion()
            for f in frames:
                c.seq_frame(f)
            c.seq_end()
            assert np.array_equal(c.process_pair(src, ref), before)
        assert c.counter(nct.CTR_ARENA_BYTES) == after


# ---- refusals

def test_refusals(wctx):
    src, ref = synth.image(*SRC), synth.image(*REF)
    with pytest.raises(nct.NctError) as e:
        wctx.seq_set_motion()
    assert e.value.code == -5 and "no sequence is open" in str(e.value)
    wctx.seq_begin(ref, src.shape)
    try:
        for kw, word in ((dict(radius0=9), "radius0"), (dict(radius0=-1), "radius0"), (dict(radius=4), "radius"), (dict(radius=-1), "radius"),
                         (dict(penalty=256), "penalty"), (dict(penalty=-1), "penalty")):
            with pytest.raises(nct.NctError) as e:
                wctx.seq_set_motion(**kw)
            assert e.value.code == -2 and word in str(e.value), str(e.value)
        assert np.array_equal(wctx.seq_frame(src), wctx_pair(wctx, src, ref))                # the sequence is still usable
    finally:
        wctx.seq_end()
    x, xp, lab, labp = seq_ref.blend_case(6, 7, 1)
    field = np.zeros((6, 7, 2), np.int16)
    with pytest.raises(nct.NctError) as e:
        wctx.seq_blend_mc_dev(x, xp, lab, labp, 0.7, 10.0, field, alias_prev=True)           # with a field, not in place into x_prev
    assert e.value.code == -2 and "alias" in str(e.value)
    a = np.ascontiguousarray(xp, np.float64).reshape(-1)
    with pytest.raises(nct.NctError) as e:                                                   # the host form: x_out == x_prev
        wctx._chk(wctx._l.nct_seq_blend_mc(wctx._h, np.ascontiguousarray(x, np.float64).reshape(-1), a, lab.reshape(-1, 3), labp.reshape(-1, 3), 6, 7, 0.7, 10.0, a, None,
                                           field.ctypes.data))
    assert e.value.code == -2 and "alias" in str(e.value)
    for R, pen, word in ((9, 1, "radius"), (-1, 1, "radius"), (1, 256, "penalty"), (1, -1, "penalty")):
        with pytest.raises(nct.NctError) as e:
            wctx.seq_motion_field(lab, labp, None, R, pen)
        assert e.value.code == -2 and word in str(e.value)
    for tau, sigma, word in ((1.0, 10.0, "tau"), (0.5, 0.0, "sigma")):
        with pytest.raises(nct.NctError) as e:
            wctx.seq_blend_mc(x, xp, lab, labp, tau, sigma, field)
        assert e.value.code == -2 and word in str(e.value)


# ---- console driver

def test_cli_motion(tmp_path, wctx, weights):
    from caffemodel_io import write_caffemodel
    ws, bs = weights
    (tmp_path / "model" / "vgg19").mkdir(parents=True)
    write_caffemodel(str(tmp_path / "model" / "vgg19" / "VGG_ILSVRC_19_layers.caffemodel"), ws, bs)
    inp = tmp_path / "in"; inp.mkdir()
    save = lambda name, img: Image.fromarray(img[..., ::-1].copy()).save(inp / name)
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))[..., ::-1]
    r = synth.image(*REF)
    f = seq_ref.pan_frames(3, SRC[1], SRC[2], step=2)
    save("r.png", r)
    for t in range(3):
        save("f%d.png" % t, f[t])
    (inp / "pairs.txt").write_text("f0.png r.png 2.0\nf1.png r.png 2.0\nf2.png r.png 2.0\n")
    p2 = nct.Params.default(); p2.bds_weight = 2.0

    def expected(**mot):
        try:
            wctx.seq_begin(r, f[0].shape, p2)
            if mot:
                wctx.seq_set_motion(**mot)
            return [wctx.seq_frame(x) for x in f]
        finally:
            wctx.seq_end()

    def run(out, *extra):
        res = subprocess.run([BIN, "-m", str(tmp_path / "model"), "-i", str(inp), "-o", str(out), "-g", "0", "-seq", "1", *extra], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout, [read(out / ("f%d_r_2.00.png" % t)) for t in range(3)]

    plain, default, wide = expected(), expected(radius0=3, radius=1, penalty=1), expected(radius0=4, radius=2, penalty=0)
    assert not np.array_equal(default[1], plain[1])                                          # motion is at work in what the files are compared with
    log, got = run(tmp_path / "o1", "-motion", "1")
    assert all(np.array_equal(a, b) for a, b in zip(got, default)) and "motion compensation (radius0 = 3, radius = 1, penalty = 1)" in log
    log, got = run(tmp_path / "o2", "-motion", "1", "-mr0", "4", "-mr", "2", "-mpen", "0")
    assert all(np.array_equal(a, b) for a, b in zip(got, wide))
    log, got = run(tmp_path / "o3")
    assert all(np.array_equal(a, b) for a, b in zip(got, plain)) and "motion compensation" not in log
