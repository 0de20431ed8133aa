"""Region tracking (SPEC §6.14) on the GPU: nct_seq_matte_warp[_dev] against the numpy rule, tracked working-size and full-resolution sequences frame by frame against
the composition of tests/seq_track_ref.py (the fields come from the CPU chain), the identities of rule 4 on the device, nct_seq_frame_auto with tracking on, the
refusals. All comparisons are equality of bytes / bit patterns."""
import numpy as np
import pytest

import nct
import region_ref
import seq_auto_ref as ar
import seq_mc_ref
import seq_ref
import seq_region_ref as sr
import seq_track_ref as tr
import synth

pytestmark = pytest.mark.gpu

H, W = 56, 64
REF = (2000, 48, 60)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
KINDS = sr.KINDS
INVALID, STATE = -2, -5


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def wctx(ctx, weights):
    ctx.vgg19_load_raw(*weights)
    return ctx


@pytest.fixture(scope="module")
def frames():
    return seq_ref.pan_frames(4, H, W, step=4)


@pytest.fixture(scope="module")
def ref():
    return synth.image(*REF)


def _params(levels=5):
    p = nct.Params.default()
    p.levels = levels
    return p


def begin(c, ref, levels=5, motion=True, **kw):
    c.seq_begin(ref, (H, W, 3), _params(levels), **kw)
    if motion:
        c.seq_set_motion(*MOT)


def matte(kind):
    return tr.rect(H, W, 16, 40, 30, 58) if kind == "rect" else region_ref.mask(kind, H, W)


def run_plan(c, frames, kinds=KINDS, mattes=None, tracking=True):
    """the frame calls a plan names; mattes[t] (None: none given) is set before frame t -> [(result, maps, matte in force or None, age)]"""
    if tracking:
        c.seq_set_region_tracking(True)
    got = []
    for t, (f, k) in enumerate(zip(frames, kinds)):
        if mattes is not None and mattes[t] is not None:
            c.seq_set_region(mattes[t])
        out, lv = c.seq_frame_propagate_levels(f) if k == "P" else c.seq_frame_levels(f, want_color=False)
        m, age = c.seq_get_region() if mattes is not None else (None, None)
        got.append((out, lv, m, age))
    return got


# ---- test 1: the seam

@pytest.mark.parametrize("case", range(len(tr.SEAM_CASES)))
def test_matte_warp_seam(ctx, case):
    """nct_seq_matte_warp and nct_seq_matte_warp_dev against the numpy rule, every field kind"""
    for kind in tr.FIELD_KINDS:
        mask, field = tr.seam_inputs(case, kind)
        exp = tr.matte_warp(mask, field)
        if kind == "zero":
            assert np.array_equal(exp, mask)
        for dev in (False, True):
            got = ctx.seq_matte_warp(mask, field, dev=dev)
            assert np.array_equal(got, exp), (kind, dev, int((got != exp).sum()))


def test_matte_warp_refusals(ctx):
    mask, field = tr.seam_inputs(4, "random")
    (h, w), (Hh, Ww) = tr.SEAM_CASES[4]
    out = np.empty_like(mask)
    m, f, o = mask.ctypes.data, field.ctypes.data, out.ctypes.data
    for name in ("nct_seq_matte_warp", "nct_seq_matte_warp_dev"):
        fn = getattr(ctx._l, name)
        call = lambda *a: (lambda: ctx._chk(fn(ctx._h, *a)))
        refused(call(None, Hh, Ww, f, h, w, o), INVALID, "mask_prev")
        refused(call(m, Hh, Ww, None, h, w, o), INVALID, "field")
        refused(call(m, Hh, Ww, f, h, w, None), INVALID, "mask_out")
        for bad in ((0, w), (h, 0), (4097, w), (h, 4097)):
            refused(call(m, 16384, 4097, f, bad[0], bad[1], o), INVALID, "field grid")
        for bad in ((16385, Ww), (Hh, 16385), (8200, 8200)):
            refused(call(m, bad[0], bad[1], f, h, w, o), INVALID, "target")
        refused(call(m, h - 1, Ww, f, h, w, o), INVALID, "smaller than the field grid")
        refused(call(m, Hh, w - 1, f, h, w, o), INVALID, "smaller than the field grid")
    refused(lambda: ctx.seq_matte_warp(mask, field, dev=True, alias=True), INVALID, "alias")


# ---- test 2: a tracked working-size sequence

_expected = {}


def expected(oracle, weights, frames, ref, kind, levels, tau):
    key = (kind, levels, tau)
    if key not in _expected:
        _expected[key] = tr.sequence(oracle, frames, [matte(kind), None, None, None], ref, *weights, kinds=KINDS, mot=MOT, levels=levels, tau=tau)
    return _expected[key]


@pytest.mark.parametrize("tau", [seq_ref.TAU, 0.0])
@pytest.mark.parametrize("kind", ["rect", "ramp"])
@pytest.mark.parametrize("levels", [5, 2])
def test_tracked_sequence(wctx, oracle, weights, frames, ref, levels, kind, tau):
    """a matte on frame 0 only, plan F B P B with motion on: the results, the matte in force with its age after every frame and level 0's kept X' against the composition
    fed the numpy-carried mattes; tau == 0: the fields are found although no frame blends"""
    exp, keeps, _, M, ages = expected(oracle, weights, frames, ref, kind, levels, tau)
    assert ages == [0, 1, 2, 3] and any(not np.array_equal(m, M[0]) for m in M)          # condition on the expected side: the matte moves
    begin(wctx, ref, levels, tau=tau)
    try:
        got = run_plan(wctx, frames, mattes=[matte(kind), None, None, None])
    finally:
        wctx.seq_end()
    for t, (out, lv, m, age) in enumerate(got):
        assert np.array_equal(m, M[t]), ("matte", t, int((m != M[t]).sum()))
        assert age == ages[t], ("age", t)
        assert np.array_equal(words(lv["ab_blend"][0]), words(keeps[t]["ab_blend"][0])), ("kept X' of level 0", t)
        assert np.array_equal(out, exp[t]), (t, KINDS[t], int((out != exp[t]).any(axis=-1).sum()))


# ---- test 3: full-resolution tracked sequences

H0, W0 = 112, 128
REF0 = (2000, 100, 120)
MAX_SIDE = 64
FULL_KINDS = "FBP"


def full_frames():
    return seq_ref.pan_frames(3, H0, W0, step=8)          # 4 px per frame at the working size 56 x 64: the two-level chain finds a field


@pytest.mark.parametrize("finish,sigma", [(nct.FINISH_EXACT, None), (nct.FINISH_UPSAMPLE, None), (nct.FINISH_UPSAMPLE, 10.0)])
def test_fullres_tracked_sequence(wctx, oracle, weights, finish, sigma):
    """the matte is carried at the original size with the working-size level's field and shrunk like nct_seq_set_region's; exact, upsampling and guided finish"""
    f0 = full_frames()
    m0 = tr.rect(H0, W0, 30, 80, 60, 116)
    exp, keeps, _, M, ages = tr.fullres_sequence(oracle, f0, [m0, None, None], synth.image(*REF0), *weights, MAX_SIDE, finish, sigma, kinds=FULL_KINDS, mot=MOT, levels=2)
    assert any(not np.array_equal(m, m0) for m in M)
    wctx.set_finish_guided(sigma)
    try:
        wctx.seq_begin_fullres(synth.image(*REF0), f0[0].shape, MAX_SIDE, finish, _params(2))
        try:
            wctx.seq_set_motion(*MOT)
            wctx.seq_set_region_tracking(True)
            wctx.seq_set_region(m0)
            for t, k in enumerate(FULL_KINDS):
                out, lv = wctx.seq_frame_propagate_levels(f0[t]) if k == "P" else wctx.seq_frame_levels(f0[t])
                m, age = wctx.seq_get_region()
                assert m.shape == (H0, W0) and np.array_equal(m, M[t]) and age == ages[t], ("matte", t)
                assert np.array_equal(words(lv["ab_blend"][0]), words(keeps[t]["ab_blend"][0])), ("kept X' of level 0", t)
                assert np.array_equal(out, exp[t]), (t, k, int((out != exp[t]).any(axis=-1).sum()))
        finally:
            wctx.seq_end()
    finally:
        wctx.set_finish_guided(None)


# ---- test 4: identities

@pytest.mark.parametrize("levels,tau", [(5, seq_ref.TAU), (2, seq_ref.TAU), (2, 0.0)])
def test_tracked_equals_the_matte_set_before_every_frame(wctx, frames, ref, levels, tau):
    """the bytes and the kept state of a tracked sequence are those of the sequence that is given M_t before every frame"""
    begin(wctx, ref, levels, tau=tau)
    try:
        tracked = run_plan(wctx, frames, mattes=[matte("ramp"), None, None, None])
    finally:
        wctx.seq_end()
    M = [g[2] for g in tracked]
    assert any(not np.array_equal(m, M[0]) for m in M)
    begin(wctx, ref, levels, tau=tau)
    try:
        manual = run_plan(wctx, frames, mattes=M, tracking=False)
    finally:
        wctx.seq_end()
    for t in range(4):
        assert np.array_equal(tracked[t][0], manual[t][0]), t
        assert manual[t][3] == 0 and np.array_equal(manual[t][2], M[t])
        for l in range(levels):
            assert np.array_equal(words(tracked[t][1]["ab_blend"][l]), words(manual[t][1]["ab_blend"][l])), (t, l)


def test_full_and_empty_mattes(wctx, frames, ref):
    """M == 255 tracked is the unmasked sequence, M == 0 tracked returns every source: a byte is copied, so both mattes stay what they are"""
    begin(wctx, ref, 2)
    try:
        plain = run_plan(wctx, frames, tracking=False)
    finally:
        wctx.seq_end()
    for kind in ("full", "empty"):
        begin(wctx, ref, 2)
        try:
            got = run_plan(wctx, frames, mattes=[matte(kind), None, None, None])
        finally:
            wctx.seq_end()
        for t in range(4):
            assert np.array_equal(got[t][2], matte(kind)) and got[t][3] == t
            assert np.array_equal(got[t][0], plain[t][0] if kind == "full" else frames[t]), (kind, t)
            if kind == "full":
                assert np.array_equal(words(got[t][1]["ab_blend"][1]), words(plain[t][1]["ab_blend"][1])), t


def test_motion_off_reset_and_a_matte_set_again(wctx, frames, ref):
    m, ramp = matte("rect"), matte("ramp")
    # motion off: the tracked sequence is the sticky one, and the age still counts
    runs = []
    for tracking in (False, True):
        begin(wctx, ref, 2, motion=False)
        try:
            runs.append(run_plan(wctx, frames, mattes=[m, None, None, None], tracking=tracking))
        finally:
            wctx.seq_end()
    for t in range(4):
        assert np.array_equal(runs[0][t][0], runs[1][t][0]) and np.array_equal(runs[1][t][2], m), t
        assert runs[0][t][3] == 0 and runs[1][t][3] == t
    # nct_seq_reset keeps the matte: the frame after it has no field, the matte stays and the age counts; a matte set again mid-clip is used as it came, age 0;
    # turning tracking off leaves the carried matte in force
    begin(wctx, ref, 2)
    try:
        wctx.seq_set_region_tracking(True)
        wctx.seq_set_region(m)
        wctx.seq_frame(frames[0]); wctx.seq_frame(frames[1]); wctx.seq_frame(frames[2])
        carried, age = wctx.seq_get_region()
        assert age == 2 and not np.array_equal(carried, m)
        wctx.seq_reset()
        after_reset = wctx.seq_frame(frames[3])
        kept, age = wctx.seq_get_region()
        assert age == 3 and np.array_equal(kept, carried)
        wctx.seq_set_region(ramp)
        again = wctx.seq_frame(frames[3])
        now, age = wctx.seq_get_region()
        assert age == 0 and np.array_equal(now, ramp)
        wctx.seq_set_region_tracking(False)
        wctx.seq_frame(frames[2])
        now, age = wctx.seq_get_region()
        assert age == 0 and np.array_equal(now, ramp)
        wctx.seq_probe(frames[1])                                          # the probe does not use a new matte up
        wctx.seq_set_region_tracking(True)
        wctx.seq_set_region(m)
        wctx.seq_probe(frames[1])
        refused(lambda: wctx.seq_frame_auto(frames[1], nct.seq_auto(threshold=-1)), INVALID, "threshold")      # nor does a refused call
        wctx.seq_frame(frames[1])
        now, age = wctx.seq_get_region()
        assert age == 0 and np.array_equal(now, m)
    finally:
        wctx.seq_end()
    prm = _params(2)
    assert np.array_equal(after_reset, wctx.process_pair_region(frames[3], carried, ref, 0, prm))
    assert not np.array_equal(again, after_reset)


@pytest.mark.parametrize("clip", ["pan", "cut"])
def test_auto_decides_as_without_tracking(wctx, ref, clip):
    """nct_seq_frame_auto's decisions and the probe's record do not depend on tracking; the frames are those of the manual calls the decisions name; on a CUT frame the
    matte stays and the age counts"""
    fr, mot, auto = ar.clips(H, W)[clip]
    au = nct.seq_auto(*auto)
    m = matte("rect")
    strip = lambda d: {k: v for k, v in d.items() if k != "probe_ms"}

    def walk(tracked):
        begin(wctx, ref, 3, motion=False)
        try:
            wctx.seq_set_motion(*mot)
            if tracked:
                wctx.seq_set_region_tracking(True)
                wctx.seq_set_region(m)
            outs, ds, mattes = [], [], []
            for f in fr:
                o, d = wctx.seq_frame_auto(f, au)
                outs.append(o); ds.append(strip(d))
                if tracked:
                    mattes.append(wctx.seq_get_region())
            manual = []
            if tracked:
                wctx.seq_reset()
                wctx.seq_set_region_tracking(False)
                for f, d, (mt, _) in zip(fr, ds, mattes):
                    wctx.seq_set_region(mt)
                    if d["kind"] == ar.SCENE_CUT:
                        wctx.seq_reset()
                    manual.append(wctx.seq_frame_propagate(f) if d["kind"] == ar.PROPAGATED else wctx.seq_frame(f))
            return outs, ds, mattes, manual
        finally:
            wctx.seq_end()
    _, plain_ds, _, _ = walk(False)
    outs, ds, mattes, manual = walk(True)
    kinds = ar.kinds(plain_ds)
    assert kinds == {"pan": "FPPKP", "cut": "FPCP"}[clip]
    assert ds == plain_ds
    assert [a for _, a in mattes] == list(range(len(fr)))
    assert all(np.array_equal(a, b) for a, b in zip(outs, manual))
    assert not np.array_equal(mattes[1][0], m)                             # the matte follows the pan
    if clip == "cut":
        t = kinds.index("C")
        assert np.array_equal(mattes[t][0], mattes[t - 1][0])


def test_untracked_sequences_keep_bytes_and_arena(wctx, frames, ref):
    """a sequence that never turns tracking on holds what an identical sequence run first held and returns its bytes — also after a tracked sequence ran"""
    m = matte("ramp")

    def sticky():
        begin(wctx, ref, 2)
        try:
            return run_plan(wctx, frames, mattes=[m, None, None, None], tracking=False)
        finally:
            wctx.seq_end()
    first = sticky()
    held = wctx.counter(nct.CTR_ARENA_BYTES)
    again = sticky()
    assert wctx.counter(nct.CTR_ARENA_BYTES) == held
    begin(wctx, ref, 2)
    try:
        tracked = run_plan(wctx, frames, mattes=[m, None, None, None])
    finally:
        wctx.seq_end()
    after = sticky()
    for t in range(4):
        for other in (again, after):
            assert np.array_equal(first[t][0], other[t][0]) and np.array_equal(other[t][2], m) and other[t][3] == 0, t
            assert all(np.array_equal(words(x), words(y)) for x, y in zip(first[t][1]["ab_blend"], other[t][1]["ab_blend"]))
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(first, tracked))


def test_tracking_refusals(wctx, frames, ref):
    refused(lambda: wctx.seq_set_region_tracking(True), STATE, "no sequence is open")
    refused(lambda: wctx.seq_get_region(), STATE, "no sequence is open")
    begin(wctx, ref, 2)
    try:
        for on in (-1, 2):
            refused(lambda: wctx._chk(wctx._l.nct_seq_set_region_tracking(wctx._h, on)), INVALID, "on must be 0 or 1")
        refused(lambda: wctx.seq_get_region(), STATE, "no region mask is set")
        wctx.seq_set_region_tracking(True)                                 # tracking on and no matte: the unmasked sequence
        wctx.seq_frame(frames[0])
        refused(lambda: wctx.seq_get_region(), STATE, "no region mask is set")
        wctx.seq_set_region(matte("rect"))
        refused(lambda: wctx._chk(wctx._l.nct_seq_get_region(wctx._h, None, None)), INVALID, "mask_out")
        out = np.empty((H, W), np.uint8)
        wctx._chk(wctx._l.nct_seq_get_region(wctx._h, out.ctypes.data, None))      # age is nullable
        assert np.array_equal(out, matte("rect"))
    finally:
        wctx.seq_end()
