"""Reference region masks in sequences (SPEC §6.19) on the GPU: k_seq_pull_hold through its two seams against the numpy rule (tests/seq_refregion_ref.py), working-size
sequences over one and two references level by level and full-resolution sequences frame by frame against the composition, the identities (a)-(e) on the device, a mask
replaced in mid-sequence, nct_seq_frame_auto, nct_pair_fit_lut and the refusals. All comparisons are equality of bytes / bit patterns."""
import numpy as np
import pytest

import nct
import region_ref
import seq_mc_ref
import seq_multi_ref
import seq_ref
import seq_refregion_ref as srr
import synth

pytestmark = pytest.mark.gpu

H, W = 56, 64
REF = (2000, 48, 60)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
KINDS = srr.KINDS


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def refused(call, code, text):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)


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
    return seq_ref.pan_frames(4, H, W)


@pytest.fixture(scope="module")
def ref():
    return synth.image(*REF)


@pytest.fixture(scope="module")
def half():
    return region_ref.mask("half", REF[1], REF[2])


def _params(levels=2):
    p = nct.Params.default()
    p.levels = levels
    return p


def begin(c, refs, levels=2, motion=True, **kw):
    if len(refs) == 1:
        c.seq_begin(refs[0], (H, W, 3), _params(levels), **kw)
    else:
        c.seq_begin_multi(refs, (H, W, 3), _params(levels), **kw)
    if motion:
        c.seq_set_motion(*MOT)


# ---- the seam

@pytest.mark.parametrize("grid", srr.GRIDS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_pull_hold_seam_matches_the_numpy_rule(ctx, grid, K):
    """nct_seq_pull_hold and its _dev form: every field kind, with and without a source mask, an unmasked reference among several, tau 0.7 and next to 1"""
    h, w = grid
    for field in (None, "zero", "random", "extreme"):
        for with_mask in (True, False):
            c = srr.hold_case(h, w, K, 1000 * K + 31 * h + w, field, with_mask, unmasked=K - 1 if K > 1 else None)
            for tau in (0.7, 1.0 - 2.0 ** -53):
                eh, em, ef = srr.pull_hold(*srr.args_of(c), tau, 10.0)
                for dev in (False, True):
                    got = ctx.seq_pull_hold(*srr.args_of(c), tau=tau, sigma=10.0, dev=dev)
                    assert got["p"].dtype == np.uint8 and np.array_equal(got["p"], eh), (field, with_mask, tau, dev)
                    assert np.array_equal(got["m"], em) and np.array_equal(got["p_free"], ef), (field, with_mask, tau, dev)
    # nullable outputs, and the free pull at tau = 0
    got = ctx.seq_pull_hold(*srr.args_of(c), tau=0.0, sigma=10.0, want=("p",))
    assert set(got) == {"p"} and np.array_equal(got["p"], ef)


def test_pull_hold_seam_refusals(ctx):
    c = srr.hold_case(9, 11, 2, 3)
    a = srr.args_of(c)
    refused(lambda: ctx.seq_pull_hold(*a, tau=1.0), -2, "tau")
    refused(lambda: ctx.seq_pull_hold(*a, tau=-0.1), -2, "tau")
    refused(lambda: ctx.seq_pull_hold(*a, sigma=0.0), -2, "sigma")
    refused(lambda: ctx.seq_pull_hold(*a, sigma=float("inf")), -2, "sigma")
    refused(lambda: ctx.seq_pull_hold(*a, shape=(0, 11)), -2, "h")
    refused(lambda: ctx.seq_pull_hold(*a, shape=(9, 4097)), -2, "w")
    refused(lambda: ctx.seq_pull_hold([c["pulled"][0]] * 9, *a[1:]), -2, "K")
    refused(lambda: ctx.seq_pull_hold(c["pulled"], None, *a[2:]), -2, "label")
    refused(lambda: ctx.seq_pull_hold(*a, dev=True, alias=True), -2, "alias")


# ---- working-size sequences level by level

_expected = {}


def expected(oracle, weights, frames, refs, qs, key, **kw):
    if key not in _expected:
        _expected[key] = srr.sequence(oracle, frames, kw.pop("masks", None), refs, qs, *weights, kinds=KINDS, **kw)
    return _expected[key]


def check_frame(lv, keep, k, levels, K, t):
    """a frame's report against the composition's keep; a propagated frame reports p_held per level run and the rest for the top level run only"""
    top = levels - 1
    for l in range(levels):
        assert np.array_equal(lv["p_held"][l], keep["p_held"][l]), ("p_held", t, l)
        assert np.array_equal(words(lv["ab_blend"][l]), words(keep["ab_blend"][l])), ("ab_blend", t, l)
        assert np.array_equal(lv["motion"][l], keep["motion"][l]), ("motion", t, l)
    if k == "P":
        assert np.array_equal(lv["mask"][top], keep["mask"]) and np.array_equal(lv["mask_full"][top], keep["mask_full"]), ("mask", t)
        assert np.array_equal(words(lv["ab_mix"][top]), words(keep["ab_mix"])), ("ab_mix", t)
        return
    for l in range(levels):
        assert np.array_equal(lv["p_free"][l], keep["p_free"][l]), ("p_free", t, l)
        assert np.array_equal(lv["mask"][l], keep["mask"][l]), ("mask", t, l)
        assert np.array_equal(lv["mask_full"][l], keep["mask_full"][l]), ("mask_full", t, l)
        assert np.array_equal(words(lv["ab_mix"][l]), words(keep["ab_mix"][l])), ("ab_mix", t, l)
        assert np.array_equal(words(lv["tau_map"][l]), words(keep["tau_map"][l])), ("tau_map", t, l)
        assert np.array_equal(lv["label"][l], keep["label"][l]), ("label", t, l)
        for r in range(K):
            if keep["pulled"][r][l] is not None:
                assert np.array_equal(lv["pulled"][r][l], keep["pulled"][r][l]), ("pulled", t, l, r)
                assert np.array_equal(lv["ref_mask"][r][l], keep["ref_mask"][r][l]), ("ref_mask", t, l, r)
        if "result" in lv:
            assert np.array_equal(lv["result"][l], keep["result"][l]), ("result", t, l)


def plain_states(c, frames, refs, levels, motion):
    """the kept X' of the sequence that never sets a mask, per frame and level"""
    begin(c, refs, levels, motion)
    try:
        return [(c.seq_frame_propagate_levels(f) if k == "P" else c.seq_frame_levels(f, want_color=False, want_levels=False))[1]["ab_blend"] for f, k in zip(frames, KINDS)]
    finally:
        c.seq_end()


@pytest.mark.parametrize("motion,levels", [(True, 2), (False, 2), (True, 5)])
def test_one_reference_half_mask_level_by_level(wctx, oracle, weights, frames, ref, half, motion, levels):
    exp, keeps, _ = expected(oracle, weights, frames, [ref], [half], ("k1", motion, levels), mot=MOT if motion else None, levels=levels)
    # conditions on the expected side: the blended frames hold (P' differs from the free pull), and the mask is partial on the source's grid
    assert any(not np.array_equal(keeps[t]["p_held"][l], keeps[t]["p_free"][l]) for t in (1, 3) for l in range(levels))
    assert 0 < (keeps[0]["p_held"][levels - 1] >= 128).mean() < 1
    plain = plain_states(wctx, frames, [ref], levels, motion)
    begin(wctx, [ref], levels, motion)
    try:
        wctx.seq_set_ref_region(0, half)
        for t, k in enumerate(KINDS):
            out, lv = wctx.seq_frame_propagate_ref_region_levels(frames[t]) if k == "P" else wctx.seq_frame_ref_region_levels(frames[t])
            check_frame(lv, keeps[t], k, levels, 1, t)
            assert np.array_equal(out, exp[t]), (t, k, int((out != exp[t]).any(axis=-1).sum()))
            assert np.array_equal(words(lv["ab_blend"][0]), words(plain[t][0])), ("identity (f)", t)      # the kept X' at level 0 is the unmasked sequence's
        # the plain entry points give the same frames
        wctx.seq_reset()
        for t, k in enumerate(KINDS):
            out = wctx.seq_frame_propagate(frames[t]) if k == "P" else wctx.seq_frame(frames[t])
            assert np.array_equal(out, exp[t]), ("plain", t)
    finally:
        wctx.seq_end()


def test_two_references_one_masked_with_a_source_mask(wctx, oracle, weights, frames, ref, half):
    """K = 2, reference 0 masked, §6.18's hold on, a source mask with protect = 1"""
    refs = [ref, seq_multi_ref.competing(ref)]
    ms = region_ref.mask("ramp", H, W)
    exp, keeps, _ = expected(oracle, weights, frames, refs, [half, None], "k2", masks=[ms] * 4, mot=MOT, levels=2, protect=1)
    assert all(min((k["label"][-1] == r).mean() for r in (0, 1)) > 0 for k in keeps)                     # both references hold a share of the finest label map
    assert any(not np.array_equal(keeps[t]["p_held"][l], keeps[t]["p_free"][l]) for t in (1, 3) for l in range(2))
    begin(wctx, refs, 2)
    try:
        wctx.seq_set_region(ms, 1)
        wctx.seq_set_ref_region(0, half)
        for t, k in enumerate(KINDS):
            out, lv = wctx.seq_frame_propagate_ref_region_levels(frames[t]) if k == "P" else wctx.seq_frame_ref_region_levels(frames[t])
            check_frame(lv, keeps[t], k, 2, 2, t)
            if k != "P":
                assert all(np.array_equal(lv["free_label"][l], keeps[t]["free_label"][l]) for l in range(2)), t
            assert np.array_equal(out, exp[t]), (t, k, int((out != exp[t]).any(axis=-1).sum()))
    finally:
        wctx.seq_end()


# ---- full-resolution sequences

REF0 = (2000, 100, 120)
H0, W0 = 112, 128
MAX_SIDE = 64
FULL_KINDS = "FBP"


@pytest.mark.parametrize("finish,sigma", [(nct.FINISH_EXACT, None), (nct.FINISH_UPSAMPLE, None), (nct.FINISH_UPSAMPLE, 10.0)])
def test_fullres_sequence(wctx, oracle, weights, finish, sigma):
    f0 = seq_ref.pan_frames(3, H0, W0, step=2)
    ref0 = synth.image(*REF0)
    q0 = region_ref.mask("half", REF0[1], REF0[2])
    m0 = region_ref.mask("ramp", H0, W0) if sigma else None                                              # the guided case also carries a source mask, protect = 1
    protect = 1 if sigma else 0
    exp, keeps, _ = srr.fullres_sequence(oracle, f0, None if m0 is None else [m0] * 3, [ref0], [q0], *weights, MAX_SIDE, finish, sigma, kinds=FULL_KINDS, mot=MOT,
                                         levels=2, protect=protect)
    wctx.set_finish_guided(sigma)
    try:
        wctx.seq_begin_fullres(ref0, f0[0].shape, MAX_SIDE, finish, _params(2))
        try:
            wctx.seq_set_motion(*MOT)
            if m0 is not None:
                wctx.seq_set_region(m0, protect)
            wctx.seq_set_ref_region(0, q0)
            for t, k in enumerate(FULL_KINDS):
                out, lv = wctx.seq_frame_propagate_ref_region_levels(f0[t]) if k == "P" else wctx.seq_frame_ref_region_levels(f0[t])
                assert out.shape == f0[t].shape
                check_frame(lv, keeps[t], k, 2, 1, t)
                assert np.array_equal(out, exp[t]), (t, k, int((out != exp[t]).any(axis=-1).sum()))
                assert not np.array_equal(out, f0[t])
            # nct_pair_fit_lut after such a frame fits over the last level's F >= 128 at the size it reads: the masked fit of (frame, result) with that F
            if finish == nct.FINISH_EXACT:
                F = keeps[2]["mask_full"]
                assert F.shape == (H0, W0) and 0 < (F >= 128).mean() < 1
                assert np.array_equal(wctx.pair_fit_lut(size=9).view(np.uint32), wctx.lut_fit_masked(f0[2], exp[2], F, size=9).view(np.uint32))
        finally:
            wctx.seq_end()
    finally:
        wctx.set_finish_guided(None)


# ---- the identities

def run_plain(c, frames, refs, levels=2, kinds=KINDS, setter=None, **kw):
    """the frames through the plain entry points -> (results, the arena's size while the sequence is open)"""
    begin(c, refs, levels, **kw)
    try:
        if setter:
            setter(c)
        outs = [c.seq_frame_propagate(f) if k == "P" else c.seq_frame(f) for f, k in zip(frames, kinds)]
        return outs, c.counter(nct.CTR_ARENA_BYTES)
    finally:
        c.seq_end()


def test_identity_a_no_setter_keeps_bytes_and_arena(weights, frames, ref, half):
    """(a): a sequence that never calls nct_seq_set_ref_region returns the bytes and holds the arena of an identical sequence run before any masked one"""
    c = nct.Context(0)
    try:
        c.vgg19_load_raw(*weights)
        refs = [ref, seq_multi_ref.competing(ref)]
        run_plain(c, frames, refs)                                  # a context's first sequence leaves cached blocks behind that its second one reuses differently
        first, held = run_plain(c, frames, refs)
        again, held2 = run_plain(c, frames, refs)
        assert held2 == held and all(np.array_equal(a, b) for a, b in zip(first, again))
        masked, _ = run_plain(c, frames, refs, setter=lambda x: x.seq_set_ref_region(0, half))
        assert not any(np.array_equal(a, b) for a, b in zip(first, masked))
        after, _ = run_plain(c, frames, refs)
        assert all(np.array_equal(a, b) for a, b in zip(first, after))
    finally:
        c.close()


def test_identities_b_and_c(wctx, frames, ref):
    full, empty = np.full(REF[1:], 255, np.uint8), np.zeros(REF[1:], np.uint8)
    refs = [ref, seq_multi_ref.competing(ref)]
    # (b): every Q == 255 — the unmasked sequence's bytes and kept state on every frame kind
    plain = plain_states(wctx, frames, refs, 2, True)
    plain_out, _ = run_plain(wctx, frames, refs)
    begin(wctx, refs, 2)
    try:
        wctx.seq_set_ref_region(0, full); wctx.seq_set_ref_region(1, full)
        for t, k in enumerate(KINDS):
            out, lv = wctx.seq_frame_propagate_ref_region_levels(frames[t]) if k == "P" else wctx.seq_frame_ref_region_levels(frames[t])
            assert np.array_equal(out, plain_out[t]), ("b", t)
            assert all(np.array_equal(words(lv["ab_blend"][l]), words(plain[t][l])) and (lv["p_held"][l] == 255).all() for l in range(2)), ("b", t)
    finally:
        wctx.seq_end()
    # (c): K = 1, Q == 0 — every frame is its source, for either protect
    for protect in (0, 1):
        outs, _ = run_plain(wctx, frames, [ref], setter=lambda x: x.seq_set_ref_region(0, empty, protect))
        assert all(np.array_equal(o, f) for o, f in zip(outs, frames)), protect


def test_identities_d_and_e(wctx, frames, ref, half):
    """(d): a first frame, a frame after a reset, a CUT frame and every frame with tau == 0 equal nct_process_pair_ref_region / nct_process_multi_ref_region; (e): with a
    source matte as well a first frame is nct_process_pair_ref_region with both masks"""
    prm = _params(2)
    pair = [wctx.process_pair_ref_region(f, None, ref, half, None, prm) for f in frames[:2]]
    begin(wctx, [ref], 2)
    try:
        wctx.seq_set_ref_region(0, half)
        first = wctx.seq_frame(frames[0])
        blended = wctx.seq_frame(frames[1])
        wctx.seq_reset()
        after_reset = wctx.seq_frame(frames[1])
        always_cut = nct.SeqAuto.default(); always_cut.cut_permille = 0
        cut, d = wctx.seq_frame_auto(frames[0], always_cut)
        assert d["kind"] == nct.SEQ_CUT
    finally:
        wctx.seq_end()
    assert np.array_equal(first, pair[0]) and np.array_equal(after_reset, pair[1]) and np.array_equal(cut, pair[0])
    assert not np.array_equal(blended, pair[1])
    outs, _ = run_plain(wctx, frames[:2], [ref], kinds="FB", tau=0.0, setter=lambda x: x.seq_set_ref_region(0, half))
    assert np.array_equal(outs[0], pair[0]) and np.array_equal(outs[1], pair[1])
    refs = [ref, seq_multi_ref.competing(ref)]
    outs, _ = run_plain(wctx, frames[:1], refs, kinds="F", setter=lambda x: x.seq_set_ref_region(1, half))
    assert np.array_equal(outs[0], wctx.process_multi_ref_region(frames[0], None, refs, [None, half], None, prm))
    # (e)
    ms = region_ref.mask("ramp", H, W)
    outs, _ = run_plain(wctx, frames[:1], [ref], kinds="F", setter=lambda x: (x.seq_set_region(ms, 1), x.seq_set_ref_region(0, half)))
    assert np.array_equal(outs[0], wctx.process_pair_ref_region(frames[0], ms, ref, half, 1, prm))


def test_identity_d_exact_finish(wctx):
    f0 = seq_ref.pan_frames(1, H0, W0, step=2)[0]
    ref0 = synth.image(*REF0)
    q0 = region_ref.mask("half", REF0[1], REF0[2])
    wctx.seq_begin_fullres(ref0, f0.shape, MAX_SIDE, nct.FINISH_EXACT, _params(2))
    try:
        wctx.seq_set_ref_region(0, q0)
        first = wctx.seq_frame(f0)
    finally:
        wctx.seq_end()
    assert np.array_equal(first, wctx.process_pair_fullres_ref_region(f0, None, ref0, q0, MAX_SIDE, None, _params(2)))


# ---- a mask replaced in mid-sequence

def test_a_mask_replaced_in_mid_sequence(wctx, oracle, weights, frames, ref, half):
    other = np.ascontiguousarray(half[:, ::-1])
    exp, keeps, _ = srr.sequence(oracle, frames[:3], None, [ref], [[half], [other], [other]], *weights, kinds="FBB", mot=MOT, levels=2)
    begin(wctx, [ref], 2)
    try:
        wctx.seq_set_ref_region(0, half)
        assert np.array_equal(wctx.seq_frame(frames[0]), exp[0])
        wctx.seq_set_ref_region(0, other)
        # a propagated frame right after the change is refused and changes nothing; nct_seq_frame_auto would have propagated and reports KEY instead
        refused(lambda: wctx.seq_frame_propagate(frames[1]), -5, "full frame")
        never_key = nct.SeqAuto.default(); never_key.cut_permille = 1001; never_key.key_permille = 1001; never_key.max_gap = 1000
        assert wctx.seq_probe(frames[1], never_key)["kind"] == nct.SEQ_PROPAGATED                     # the probe does not look at the masks
        out, lv = wctx.seq_frame_ref_region_levels(frames[1])
        assert np.array_equal(out, exp[1])
        assert all(np.array_equal(lv["p_held"][l], lv["p_free"][l]) and np.array_equal(lv["p_held"][l], keeps[1]["p_held"][l]) for l in range(2))
        out, lv = wctx.seq_frame_ref_region_levels(frames[2])                                          # the next full frame holds again
        assert np.array_equal(out, exp[2]) and any(not np.array_equal(lv["p_held"][l], lv["p_free"][l]) for l in range(2))
        wctx.seq_set_ref_region(0, half)
        out, d = wctx.seq_frame_auto(frames[3], never_key)
        assert d["kind"] == nct.SEQ_KEY
        out, d = wctx.seq_frame_auto(frames[3], never_key)
        assert d["kind"] == nct.SEQ_PROPAGATED
        # removed: the sequence runs unmasked, and a propagated frame needs no full frame first
        wctx.seq_set_ref_region(0, None)
        wctx.seq_frame_propagate(frames[3])
    finally:
        wctx.seq_end()


# ---- refusals

def test_refusals(wctx, frames, ref, half):
    refused(lambda: wctx.seq_set_ref_region(0, half), -5, "no sequence is open")
    begin(wctx, [ref], 2)
    try:
        refused(lambda: wctx.seq_frame_ref_region_levels(frames[0]), -5, "no reference mask is set")
        refused(lambda: wctx.seq_set_ref_region(1, half), -2, "k = 1")
        refused(lambda: wctx.seq_set_ref_region(-1, half), -2, "k = -1")
        refused(lambda: wctx.seq_set_ref_region(0, half, 2), -2, "protect")
        refused(lambda: wctx.seq_set_ref_region(0, half[:-1]), -2, "mask")
        refused(lambda: wctx.pair_set_ref_region(0, half), -5, "sequence is open")
        # the refused calls left the setting as it was: no mask, and the frame is the unmasked one
        first = wctx.seq_frame(frames[0])
        refused(lambda: wctx.seq_frame_propagate_ref_region_levels(frames[1]), -5, "no reference mask is set")
        wctx.seq_set_ref_region(0, half)
        refused(lambda: wctx.seq_frame_propagate(frames[1]), -5, "full frame")
    finally:
        wctx.seq_end()
    assert np.array_equal(first, wctx.process_pair(frames[0], ref, _params(2)))
