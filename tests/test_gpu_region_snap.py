"""Matte snapping (SPEC §6.15) on the GPU: nct_region_snap[_dev] against the numpy rule over every seam case, tracked and snapped working-size and full-resolution
sequences frame by frame against the composition of tests/region_snap_ref.py (the fields come from the CPU chain), nct_seq_frame_auto with snapping on, the
identities of rule 4 on the device, the refusals. All comparisons are equality of bytes / bit patterns."""
import ctypes as C

import numpy as np
import pytest

import nct
import region_ref
import region_snap_ref as rs
import seq_auto_ref as ar
import seq_mc_ref
import seq_ref
import seq_region_ref as sr
import seq_track_ref as tr
import synth

pytestmark = pytest.mark.gpu

H, W = 56, 64                    # the smallest frames of the sequence tests (tests/test_gpu_seq_track.py)
REF = (2000, 48, 60)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
SNAP = (rs.RADIUS, rs.SIGMA, rs.BINARY)
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
def clip():
    """the object clip at 4 px per frame -> (frames, truth mattes)"""
    return rs.obj_frames(4, H, W, 4)


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


def run_plan(c, frames, kinds=KINDS, mattes=None, tracking=True, snap=SNAP):
    """the frame calls a plan names; mattes[t] (None: none given) is set before frame t; snap: the parameters, or None to leave snapping alone
    -> [(result, maps, matte in force or None, age)]"""
    if tracking:
        c.seq_set_region_tracking(True)
    if snap is not None:
        c.seq_set_region_snap(True, *snap)
    got = []
    for t, (f, k) in enumerate(zip(frames, kinds)):
        if mattes is not None and mattes[t] is not None:
            c.seq_set_region(mattes[t])
        out, lv = c.seq_frame_propagate_levels(f) if k == "P" else c.seq_frame_levels(f, want_color=False)
        m, age = c.seq_get_region() if mattes is not None else (None, None)
        got.append((out, lv, m, age))
    return got


# ---- test 1: the seam

def snap_dev_checked(ctx, mask, lab, r, sigma, binary, shift=0):
    """nct_region_snap_dev on arena blocks, out of place: -> (the output, the two inputs as the call left them). shift: the output starts that many bytes into its
    block (shift % 4 != 0: the byte-store path also where W % 4 == 0)"""
    Hh, Ww = mask.shape
    sp = nct.RegionSnapParams.default()
    sp.radius, sp.sigma, sp.binary = r, sigma, binary
    with ctx.blocks() as b:
        blocks = [b.up(mask), b.up(lab), b.up(np.full(mask.size + 8, 0x5a, np.uint8))]
        ctx._chk(ctx._l.nct_region_snap_dev(ctx._h, blocks[0], blocks[1], Hh, Ww, C.addressof(sp), blocks[2] + shift))
        whole = ctx.dev_download(blocks[2], (mask.size + 8,), np.uint8)
        return whole, ctx.dev_download(blocks[0], mask.shape, np.uint8), ctx.dev_download(blocks[1], lab.shape, np.uint8)


@pytest.mark.parametrize("r", rs.RADII)
@pytest.mark.parametrize("case", range(len(rs.SEAM_CASES)))
def test_region_snap_seam(ctx, case, r):
    """nct_region_snap and nct_region_snap_dev against the numpy rule: every matte and guide kind, sigma and binary; the _dev form leaves its inputs and the bytes around
    its output alone, with an aligned and an unaligned output"""
    for mk in rs.MATTE_KINDS:
        for gk in rs.GUIDE_KINDS:
            mask, lab = rs.seam_inputs(case, mk, gk)
            for sigma in rs.SIGMAS:
                for binary in rs.BINARIES:
                    key = (mk, gk, sigma, binary)
                    exp = rs.snap(mask, lab, r, sigma, binary)
                    got = ctx.region_snap(mask, lab, r, sigma, binary)
                    assert np.array_equal(got, exp), (key, "host", int((got != exp).sum()))
                    got = ctx.region_snap(mask, lab, r, sigma, binary, dev=True)
                    assert np.array_equal(got, exp), (key, "dev", int((got != exp).sum()))
            # out of place, once per matte and guide kind: an unaligned output takes the byte-store path
            for shift in (0, 3):
                whole, m_after, l_after = snap_dev_checked(ctx, mask, lab, r, 10, 0, shift)
                exp = rs.snap(mask, lab, r, 10, 0)
                assert np.array_equal(whole[shift:shift + mask.size].reshape(mask.shape), exp), (mk, gk, shift)
                assert (whole[:shift] == 0x5a).all() and (whole[shift + mask.size:] == 0x5a).all(), (mk, gk, shift)
                assert np.array_equal(m_after, mask) and np.array_equal(l_after, lab), (mk, gk, shift)


def test_region_snap_defaults(ctx):
    """params == NULL: radius 3, sigma 10, binary 1"""
    mask, lab = rs.seam_inputs(4, "random", "regions")
    out = np.empty_like(mask)
    ctx._chk(ctx._l.nct_region_snap(ctx._h, mask.ctypes.data, lab.ctypes.data, mask.shape[0], mask.shape[1], None, out.ctypes.data))
    assert np.array_equal(out, rs.snap(mask, lab)) and np.array_equal(out, ctx.region_snap(mask, lab))
    assert not np.array_equal(out, np.where(mask >= 128, 255, 0))             # condition: the pass did something


def test_region_snap_refusals(ctx):
    mask, lab = rs.seam_inputs(4, "random", "random")
    Hh, Ww = mask.shape
    out = np.empty_like(mask)
    m, g, o = mask.ctypes.data, lab.ctypes.data, out.ctypes.data

    def prm(r=3, sigma=10, binary=1):
        p = nct.RegionSnapParams()
        p.radius, p.sigma, p.binary = r, sigma, binary
        return p
    for name in ("nct_region_snap", "nct_region_snap_dev"):
        fn = getattr(ctx._l, name)
        call = lambda *a: (lambda: ctx._chk(fn(ctx._h, *a)))
        refused(call(None, g, Hh, Ww, None, o), INVALID, "null mask")
        refused(call(m, None, Hh, Ww, None, o), INVALID, "null lab")
        refused(call(m, g, Hh, Ww, None, None), INVALID, "null mask_out")
        for bad in ((0, Ww), (Hh, 0), (-1, Ww), (16385, Ww), (Hh, 16385), (8200, 8200)):
            refused(call(m, g, bad[0], bad[1], None, o), INVALID, "size H x W")
        for p, word in ((prm(r=0), "radius"), (prm(r=9), "radius"), (prm(sigma=0), "sigma"), (prm(sigma=256), "sigma"), (prm(binary=2), "binary"), (prm(binary=-1), "binary")):
            refused(call(m, g, Hh, Ww, C.addressof(p), o), INVALID, word)
    refused(lambda: ctx.region_snap(mask, lab, dev=True, alias="mask"), INVALID, "alias mask")
    refused(lambda: ctx.region_snap(mask, lab, dev=True, alias="lab"), INVALID, "alias lab")


# ---- test 2: tracked and snapped working-size sequences

@pytest.mark.parametrize("levels", [5, 3])
def test_snapped_sequence(wctx, oracle, weights, clip, ref, levels):
    """a loose matte around the object on frame 0 only (2 px too wide: the carry alone keeps it loose, the snap draws it onto the object), plan F B P B with motion on:
    the results, the matte in force with its age after every frame and every level's kept X' against the composition fed the numpy-carried and -snapped mattes"""
    frames, truth = clip
    mattes = [tr.rect(H, W, 14, 42, 8, 40), None, None, None]
    exp, keeps, _, M, ages = rs.sequence(oracle, frames, mattes, ref, *weights, SNAP, kinds=KINDS, mot=MOT, levels=levels)
    plain, _ = tr.carried(oracle, frames, mattes, MOT, levels)
    assert ages == [0, 1, 2, 3] and any(not np.array_equal(a, b) for a, b in zip(M, plain))          # condition on the expected side: the snap changes the carried matte
    begin(wctx, ref, levels)
    try:
        got = run_plan(wctx, frames, mattes=mattes)
    finally:
        wctx.seq_end()
    for t, (out, lv, m, age) in enumerate(got):
        assert np.array_equal(m, M[t]), ("matte", t, int((m != M[t]).sum()))
        assert age == ages[t], ("age", t)
        for l in range(levels):
            assert np.array_equal(words(lv["ab_blend"][l]), words(keeps[t]["ab_blend"][l])), ("kept X'", t, l)
        assert np.array_equal(out, exp[t]), (t, KINDS[t], int((out != exp[t]).any(axis=-1).sum()))


def test_snapped_motion_off(wctx, oracle, clip, ref):
    """motion off: the field is zero, the snap alone re-fits the matte on every frame behind its own"""
    frames, truth = clip
    mattes = [truth[0], None, None, None]
    M, ages = rs.carried_snapped(oracle, frames, mattes, None, 2, SNAP)
    assert not np.array_equal(M[1], M[0])
    begin(wctx, ref, 2, motion=False)
    try:
        got = run_plan(wctx, frames, mattes=mattes)
    finally:
        wctx.seq_end()
    for t in range(4):
        assert np.array_equal(got[t][2], M[t]) and got[t][3] == ages[t], t


@pytest.mark.parametrize("which", ["pan", "cut"])
def test_snapped_auto(wctx, oracle, ref, which):
    """nct_seq_frame_auto with tracking and snapping on: the decisions are those without either; the mattes are the composition's, with no carry and no snap on a CUT
    frame; the frames are those of the manual calls the decisions name, each given the snapped matte"""
    fr, mot, auto = ar.clips(H, W)[which]
    au = nct.seq_auto(*auto)
    m = tr.rect(H, W, 16, 40, 30, 58)
    strip = lambda d: {k: v for k, v in d.items() if k != "probe_ms"}
    begin(wctx, ref, 3, motion=False)
    try:
        wctx.seq_set_motion(*mot)
        plain_ds = [strip(wctx.seq_frame_auto(f, au)[1]) for f in fr]
    finally:
        wctx.seq_end()
    kinds = ar.kinds(plain_ds)
    assert kinds == {"pan": "FPPKP", "cut": "FPCP"}[which]
    cuts = tuple(t for t, k in enumerate(kinds) if k == "C")
    M, ages = rs.carried_snapped(oracle, fr, [m] + [None] * (len(fr) - 1), mot, 3, SNAP, zero_at=cuts)
    begin(wctx, ref, 3, motion=False)
    try:
        wctx.seq_set_motion(*mot)
        wctx.seq_set_region_tracking(True)
        wctx.seq_set_region_snap(True, *SNAP)
        wctx.seq_set_region(m)
        outs = []
        for t, f in enumerate(fr):
            o, d = wctx.seq_frame_auto(f, au)
            assert strip(d) == plain_ds[t], t
            got, age = wctx.seq_get_region()
            assert np.array_equal(got, M[t]) and age == ages[t], ("matte", t)
            outs.append(o)
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
    for t in cuts:
        assert np.array_equal(M[t], M[t - 1])


# ---- test 3: full-resolution sequences, the snap at the original size

H0, W0 = 112, 128
REF0 = (2000, 100, 120)
MAX_SIDE = 64
FULL_KINDS = "FBP"


@pytest.mark.parametrize("finish,sigma", [(nct.FINISH_EXACT, None), (nct.FINISH_UPSAMPLE, None), (nct.FINISH_UPSAMPLE, 10.0)])
def test_fullres_snapped_sequence(wctx, oracle, weights, finish, sigma):
    """the matte is carried and snapped at the original size, the guide is the original frame in Lab; then it is shrunk like nct_seq_set_region's; exact, upsampling and
    guided finish"""
    f0, truth0 = rs.obj_frames(3, H0, W0, 8)               # 4 px per frame at the working size 56 x 64
    mattes = [truth0[0], None, None]
    exp, keeps, _, M, ages = rs.fullres_sequence(oracle, f0, mattes, synth.image(*REF0), *weights, MAX_SIDE, finish, SNAP, sigma, kinds=FULL_KINDS, mot=MOT, levels=2)
    S = [oracle.resize_u8c3(f, H, W) for f in f0]
    plain, _ = tr.carried(oracle, S, mattes, MOT, 2)
    assert any(not np.array_equal(a, b) for a, b in zip(M, plain))
    wctx.set_finish_guided(sigma)
    try:
        wctx.seq_begin_fullres(synth.image(*REF0), f0[0].shape, MAX_SIDE, finish, _params(2))
        try:
            wctx.seq_set_motion(*MOT)
            wctx.seq_set_region_tracking(True)
            wctx.seq_set_region_snap(True, *SNAP)
            wctx.seq_set_region(truth0[0])
            for t, k in enumerate(FULL_KINDS):
                out, lv = wctx.seq_frame_propagate_levels(f0[t]) if k == "P" else wctx.seq_frame_levels(f0[t])
                m, age = wctx.seq_get_region()
                assert m.shape == (H0, W0) and np.array_equal(m, M[t]) and age == ages[t], ("matte", t)
                for l in range(2):
                    assert np.array_equal(words(lv["ab_blend"][l]), words(keeps[t]["ab_blend"][l])), ("kept X'", t, l)
                assert np.array_equal(out, exp[t]), (t, k, int((out != exp[t]).any(axis=-1).sum()))
        finally:
            wctx.seq_end()
    finally:
        wctx.set_finish_guided(None)


# ---- test 4: identities

def test_snapped_equals_the_matte_set_before_every_frame(wctx, clip, ref):
    """the bytes and the kept state of a tracked and snapped sequence are those of the sequence that is given M_t before every frame"""
    frames, truth = clip
    begin(wctx, ref, 3)
    try:
        snapped = run_plan(wctx, frames, mattes=[truth[0], None, None, None])
    finally:
        wctx.seq_end()
    M = [g[2] for g in snapped]
    begin(wctx, ref, 3)
    try:
        manual = run_plan(wctx, frames, mattes=M, tracking=False, snap=None)
    finally:
        wctx.seq_end()
    for t in range(4):
        assert np.array_equal(snapped[t][0], manual[t][0]), t
        assert manual[t][3] == 0 and np.array_equal(manual[t][2], M[t])
        for l in range(3):
            assert np.array_equal(words(snapped[t][1]["ab_blend"][l]), words(manual[t][1]["ab_blend"][l])), (t, l)


def test_snap_acts_only_on_a_tracked_matte(wctx, clip, ref):
    """snapping on but tracking off, or no matte set: the sequence's bytes of before. All-255 tracked and snapped: the unmasked sequence. nct_seq_set_region_snap(NULL):
    plain tracking's bytes — and what the context holds after a sequence that never snapped does not depend on a snapped one having run"""
    frames, truth = clip
    m = region_ref.mask("ramp", H, W)

    def run(mattes, tracking, snap, off_again=False):
        begin(wctx, ref, 2)
        try:
            if off_again:
                wctx.seq_set_region_snap(True, *SNAP)
                wctx.seq_set_region_snap(False)
            return run_plan(wctx, frames, mattes=mattes, tracking=tracking, snap=snap)
        finally:
            wctx.seq_end()
    given = [m, None, None, None]
    sticky, plain = run(given, False, None), run(None, False, None)
    tracked = run(given, True, None)
    held = wctx.counter(nct.CTR_ARENA_BYTES)
    tracked_again = run(given, True, None)
    assert wctx.counter(nct.CTR_ARENA_BYTES) == held
    snapped = run(given, True, SNAP)
    assert not all(np.array_equal(a[2], b[2]) for a, b in zip(tracked, snapped))          # condition: the snap does change this matte
    cases = {"tracking off": (run(given, False, SNAP), sticky), "no matte": (run(None, True, SNAP), plain), "turned off again": (run(given, True, None, off_again=True), tracked),
             "tracked again": (tracked_again, tracked), "tracked after a snapped sequence": (run(given, True, None), tracked)}
    for name, (got, want) in cases.items():
        for t in range(4):
            assert np.array_equal(got[t][0], want[t][0]), (name, t)
            assert got[t][3] == want[t][3] and (want[t][2] is None or np.array_equal(got[t][2], want[t][2])), (name, "matte", t)
            assert all(np.array_equal(words(x), words(y)) for x, y in zip(got[t][1]["ab_blend"], want[t][1]["ab_blend"])), (name, "kept X'", t)
    full = run([np.full((H, W), 255, np.uint8), None, None, None], True, SNAP)
    for t in range(4):
        assert (full[t][2] == 255).all() and full[t][3] == t
        assert np.array_equal(full[t][0], plain[t][0]), ("all-255", t)
        assert np.array_equal(words(full[t][1]["ab_blend"][1]), words(plain[t][1]["ab_blend"][1])), ("all-255", t)


def test_reset_first_frame_and_a_new_matte_do_not_snap(wctx, clip, ref):
    frames, truth = clip
    begin(wctx, ref, 2)
    try:
        wctx.seq_set_region_tracking(True)
        wctx.seq_set_region_snap(True, *SNAP)
        m0 = tr.rect(H, W, 14, 42, 8, 40)                                 # wider than the object: frame 1's snap pulls it in
        wctx.seq_set_region(m0)
        wctx.seq_frame(frames[0])
        own, age = wctx.seq_get_region()
        assert age == 0 and np.array_equal(own, m0)                        # the matte's own frame (also a first frame) uses it as it came
        wctx.seq_frame(frames[1])
        snapped, age = wctx.seq_get_region()
        assert age == 1 and not np.array_equal(snapped, m0)
        wctx.seq_reset()
        after_reset = wctx.seq_frame(frames[2])
        kept, age = wctx.seq_get_region()
        assert age == 2 and np.array_equal(kept, snapped)                  # no state: no carry and no snap, the age counts
        wctx.seq_set_region(m0)
        wctx.seq_frame(frames[3])
        now, age = wctx.seq_get_region()
        assert age == 0 and np.array_equal(now, m0)                        # a matte set again mid-clip is used as it came
    finally:
        wctx.seq_end()
    assert np.array_equal(after_reset, wctx.process_pair_region(frames[2], snapped, ref, 0, _params(2)))


def test_seq_set_region_snap_refusals(wctx, clip, ref):
    frames, truth = clip
    refused(lambda: wctx.seq_set_region_snap(True), STATE, "no sequence is open")
    refused(lambda: wctx.seq_set_region_snap(False), STATE, "no sequence is open")
    mattes = [truth[0], None, None, None]
    begin(wctx, ref, 2)
    try:
        want = run_plan(wctx, frames[:2], mattes=mattes, snap=(1, 10, 1))
    finally:
        wctx.seq_end()
    begin(wctx, ref, 2)
    try:
        wctx.seq_set_region_snap(True, 1, 10, 1)
        for bad, word in (((0, 10, 1), "radius"), ((9, 10, 1), "radius"), ((3, 0, 1), "sigma"), ((3, 256, 1), "sigma"), ((3, 10, 2), "binary")):
            refused(lambda: wctx.seq_set_region_snap(True, *bad), INVALID, word)
        got = run_plan(wctx, frames[:2], mattes=mattes, snap=None)          # a refused call leaves the setting as it was: radius 1
    finally:
        wctx.seq_end()
    assert not np.array_equal(want[1][2], truth[0])
    for t in range(2):
        assert np.array_equal(got[t][2], want[t][2]) and np.array_equal(got[t][0], want[t][0]), t
