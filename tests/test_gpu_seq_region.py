"""Region masks in sequences (SPEC §6.13) on the GPU: the four masked finish seams against the numpy chain, a working-size masked sequence level by level and
full-resolution sequences frame by frame against the composition of tests/seq_region_ref.py, the identities of rule 5 on the device, nct_seq_frame_auto with a
mask, nct_pair_fit_lut after a masked frame, the refusals and the life of the mask. All comparisons are equality of bytes / bit patterns."""
import numpy as np
import pytest

import nct
import region_ref
import seq_auto_ref as ar
import seq_mc_ref
import seq_ref
import seq_region_ref as sr
import synth

pytestmark = pytest.mark.gpu

H, W = 56, 64
REF = (2000, 48, 60)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
KINDS = sr.KINDS


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


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


def _params(levels=5, cube=False):
    p = nct.Params.default()
    p.levels = levels
    if cube:
        p.flags |= nct.FLAG_LAB2BGR_CUBE
    return p


def begin(c, ref, levels=5, motion=True, **kw):
    c.seq_begin(ref, (H, W, 3), _params(levels), **kw)
    if motion:
        c.seq_set_motion(*MOT)


def run_kinds(c, frames, kinds=KINDS, masks=None, protect=None, region_levels=False):
    """the frame calls a plan names; masks (a list, or None: never set) are set before their frame -> [(result, maps or None)]"""
    outs = []
    for t, (f, k) in enumerate(zip(frames, kinds)):
        if masks is not None:
            c.seq_set_region(masks[t], protect)
        if region_levels:
            outs.append(c.seq_frame_propagate_region_levels(f) if k == "P" else c.seq_frame_region_levels(f, want_color=False))
        else:
            outs.append(c.seq_frame_propagate_levels(f) if k == "P" else c.seq_frame_levels(f, want_color=False))
    return outs


# ---- test 1: the four seams

@pytest.mark.parametrize("case", range(len(sr.SEAM_CASES)))
def test_masked_finish_seams(ctx, oracle, case):
    """nct_color_finish_{upsample,guided}_region[_dev] against the numpy chain: host and _dev forms, both Lab -> BGR forms, protect 0 and 1, with every outcome of the
    compose present in the inputs"""
    ab, lab_w, h, w, s_full, mask = sr.seam_inputs(oracle, case)
    for guided in (False, True):
        for protect in (0, 1):
            for form in (0, 1):
                prm = _params(cube=bool(form))
                exp, olab = sr.masked_finish(oracle, ab, h, w, s_full, mask, protect, form, lab_w if guided else None)
                by_protect, unmoved, converted = sr.outcome_shares(oracle, olab, s_full, mask, protect)
                shares = region_ref.compose_shares(oracle.bgr2lab(s_full), olab, mask)
                assert shares[1] > 0 and unmoved > 0 and converted > 0 and (mask == 0).any() and (by_protect > 0 or not protect)      # not vacuous
                for dev in (False, True):
                    if guided:
                        got = ctx.color_finish_guided_region(ab, lab_w, h, w, s_full, mask, protect, None, prm, dev=dev)
                    else:
                        got = ctx.color_finish_upsample_region(ab, h, w, s_full, mask, protect, prm, dev=dev)
                    assert np.array_equal(got, exp), (guided, protect, form, dev, int((got != exp).any(axis=-1).sum()))
    # M = 255 everywhere equals the unmasked seam, and so does a NULL mask
    full = np.full(mask.shape, 255, np.uint8)
    for protect in (0, 1):
        assert np.array_equal(ctx.color_finish_upsample_region(ab, h, w, s_full, full, protect), ctx.color_finish_upsample(ab, h, w, s_full))
        assert np.array_equal(ctx.color_finish_guided_region(ab, lab_w, h, w, s_full, full, protect), ctx.color_finish_guided(ab, lab_w, h, w, s_full))
    assert np.array_equal(ctx.color_finish_upsample_region(ab, h, w, s_full, None), ctx.color_finish_upsample(ab, h, w, s_full))
    assert np.array_equal(ctx.color_finish_guided_region_dev(ab, lab_w, h, w, s_full, None), ctx.color_finish_guided(ab, lab_w, h, w, s_full))
    # a NaN coefficient under M == 0 with protect = 1 returns the source bytes
    nan = np.full_like(ab, np.nan)
    empty = np.zeros(mask.shape, np.uint8)
    assert np.array_equal(ctx.color_finish_upsample_region(nan, h, w, s_full, empty, 1), s_full)
    assert np.array_equal(ctx.color_finish_guided_region(nan, lab_w, h, w, s_full, empty, 1), s_full)


def test_masked_finish_seam_refusals(ctx, oracle):
    ab, lab_w, h, w, s_full, mask = sr.seam_inputs(oracle, 0)
    for protect in (-1, 2):
        for call in (lambda: ctx.color_finish_upsample_region(ab, h, w, s_full, mask, protect), lambda: ctx.color_finish_upsample_region_dev(ab, h, w, s_full, mask, protect),
                     lambda: ctx.color_finish_guided_region(ab, lab_w, h, w, s_full, mask, protect), lambda: ctx.color_finish_guided_region_dev(ab, lab_w, h, w, s_full, mask, protect)):
            refused(call, -2, "protect")
    refused(lambda: ctx.color_finish_upsample_region(ab, h, w, s_full, mask[:-1]), -2, "mask")
    small = s_full[: h - 1, : w - 1]
    refused(lambda: ctx.color_finish_upsample_region(ab, h, w, small, mask[: h - 1, : w - 1]), -2, "smaller than the grid")
    refused(lambda: ctx.color_finish_guided_region(ab, lab_w, h, w, s_full, mask, 0, sigma=0.0), -2, "sigma")


# ---- test 2: a working-size masked sequence level by level

_expected = {}


def expected(oracle, weights, frames, ref, mask_kind, motion, levels, protect=0):
    key = (mask_kind, motion, levels, protect)
    if key not in _expected:
        m = region_ref.mask(mask_kind, H, W)
        _expected[key] = sr.sequence(oracle, frames, [m] * 4, ref, *weights, kinds=KINDS, mot=MOT if motion else None, levels=levels, protect=protect)
    return _expected[key]


# levels 5 where the pan's field is found (the fine levels); the other combinations at 2 levels: the same calls, the reference at a quarter of the cost
@pytest.mark.parametrize("mask_kind,motion,levels", [("half", True, 5), ("ramp", False, 2), ("half", False, 2), ("ramp", True, 2)])
def test_masked_sequence_level_by_level(wctx, oracle, weights, frames, ref, mask_kind, motion, levels):
    exp, keeps, _ = expected(oracle, weights, frames, ref, mask_kind, motion, levels)
    m = region_ref.mask(mask_kind, H, W)
    if motion and levels == 5:
        assert any(f.any() for f in keeps[1]["motion"]) and any(f.any() for f in keeps[2]["motion"])          # condition on the expected side: a field is found
    begin(wctx, ref, levels, motion)
    try:
        wctx.seq_set_region(m)
        for t, k in enumerate(KINDS):
            if k == "P":
                out, lv = wctx.seq_frame_propagate_region_levels(frames[t])
                assert np.array_equal(words(lv["ab_mix"][levels - 1]), words(keeps[t]["ab_mix"])), ("ab_mix", t)
                assert np.array_equal(lv["mask"][levels - 1], keeps[t]["mask"]), ("mask", t)
            else:
                out, lv = wctx.seq_frame_region_levels(frames[t], want_color=False)
                for l in range(levels):
                    assert np.array_equal(lv["result"][l], keeps[t]["result"][l]), ("result", t, l)
                    assert np.array_equal(words(lv["ab_mix"][l]), words(keeps[t]["ab_mix"][l])), ("ab_mix", t, l)
                    assert np.array_equal(lv["mask"][l], keeps[t]["mask"][l]), ("mask", t, l)
            for l in range(levels):
                assert np.array_equal(words(lv["ab_blend"][l]), words(keeps[t]["ab_blend"][l])), ("ab_blend", t, l)      # the unmixed kept state
                assert np.array_equal(lv["motion"][l], keeps[t]["motion"][l]), ("motion", t, l)
            assert np.array_equal(out, exp[t]), (t, k)
    finally:
        wctx.seq_end()


# ---- test 3: the identities of rule 5 on the device

def unmasked(c, frames, ref, levels, motion=True, **kw):
    begin(c, ref, levels, motion, **kw)
    try:
        return run_kinds(c, frames)
    finally:
        c.seq_end()


def test_identity_a_no_mask_keeps_bytes_and_arena(wctx, frames, ref):
    """(a): a sequence that never calls nct_seq_set_region holds what an identical sequence run first held, and returns its bytes — also after a masked sequence ran"""
    first = unmasked(wctx, frames, ref, 2)
    held = wctx.counter(nct.CTR_ARENA_BYTES)
    again = unmasked(wctx, frames, ref, 2)
    assert wctx.counter(nct.CTR_ARENA_BYTES) == held
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(first, again))
    begin(wctx, ref, 2)
    try:
        run_kinds(wctx, frames, masks=[region_ref.mask("ramp", H, W)] * 4)
    finally:
        wctx.seq_end()
    after = unmasked(wctx, frames, ref, 2)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(first, after))
    assert all(np.array_equal(words(x), words(y)) for a, b in zip(first, after) for x, y in zip(a[1]["ab_blend"], b[1]["ab_blend"]))


@pytest.mark.parametrize("levels", [5, 2])
def test_identities_b_c_e_full_empty_and_changing_masks(wctx, frames, ref, levels):
    plain = unmasked(wctx, frames, ref, levels)
    changing = [region_ref.mask(k, H, W) for k in ("half", "ramp", "random", "half")]
    for protect in (0, 1):
        # (b): M = 255 — the unmasked sequence's bytes and state, every frame kind
        begin(wctx, ref, levels)
        try:
            got = run_kinds(wctx, frames, masks=[region_ref.mask("full", H, W)] * 4, protect=protect, region_levels=True)
        finally:
            wctx.seq_end()
        for t in range(4):
            assert np.array_equal(got[t][0], plain[t][0]), ("b", protect, t)
            for l in range(levels):
                assert np.array_equal(words(got[t][1]["ab_blend"][l]), words(plain[t][1]["ab_blend"][l])), ("b", protect, t, l)
        # (c): M = 0 — every frame is its source; (e): level 0's kept X' is the unmasked sequence's
        for which, masks in (("empty", [region_ref.mask("empty", H, W)] * 4), ("changing", changing)):
            begin(wctx, ref, levels)
            try:
                got = run_kinds(wctx, frames, masks=masks, protect=protect)
            finally:
                wctx.seq_end()
            for t in range(4):
                if which == "empty":
                    assert np.array_equal(got[t][0], frames[t]), ("c", protect, t)
                else:
                    assert not np.array_equal(got[t][0], plain[t][0]) and not np.array_equal(got[t][0], frames[t])
                assert np.array_equal(words(got[t][1]["ab_blend"][0]), words(plain[t][1]["ab_blend"][0])), ("e", which, protect, t)
            assert not np.array_equal(words(got[0][1]["ab_blend"][levels - 1]), words(plain[0][1]["ab_blend"][levels - 1]))      # (e) is a statement about level 0


def test_identity_d_frames_that_equal_the_masked_pair(wctx, frames, ref):
    levels, prm = 2, _params(2)
    masks = [region_ref.mask(k, H, W) for k in ("half", "ramp")]
    begin(wctx, ref, levels)
    try:
        wctx.seq_set_region(masks[0], 1)
        first = wctx.seq_frame(frames[0])
        wctx.seq_set_region(masks[1], 0)
        blended = wctx.seq_frame(frames[1])
        wctx.seq_reset()
        after_reset = wctx.seq_frame(frames[1])
    finally:
        wctx.seq_end()
    begin(wctx, ref, levels, tau=0.0)
    try:
        wctx.seq_set_region(masks[0], 1)
        tau0 = [wctx.seq_frame(frames[0])]
        wctx.seq_set_region(masks[1], 0)
        tau0.append(wctx.seq_frame(frames[1]))
    finally:
        wctx.seq_end()
    pair = [wctx.process_pair_region(frames[0], masks[0], ref, 1, prm), wctx.process_pair_region(frames[1], masks[1], ref, 0, prm)]
    assert np.array_equal(first, pair[0]) and np.array_equal(after_reset, pair[1])
    assert not np.array_equal(blended, pair[1])
    assert np.array_equal(tau0[0], pair[0]) and np.array_equal(tau0[1], pair[1])


@pytest.mark.parametrize("levels,mot", [(5, MOT), (2, None)])
def test_identity_g_identical_frame_with_the_same_mask(wctx, frames, ref, levels, mot):
    m = region_ref.mask("ramp", H, W)
    begin(wctx, ref, levels, motion=mot is not None)
    try:
        wctx.seq_set_region(m)
        wctx.seq_frame(frames[0])
        prev = wctx.seq_frame(frames[1])
        for _ in range(2):                                                 # after a full frame, then after a propagated one
            assert np.array_equal(wctx.seq_frame_propagate(frames[1]), prev)
        assert not np.array_equal(wctx.seq_frame_propagate(frames[2]), prev)
    finally:
        wctx.seq_end()


# ---- test 4: full-resolution sequences

REF0 = (2000, 100, 120)
MAX_SIDE = 64
FULL_KINDS = "FBP"


def full_frames(h0, w0):
    return seq_ref.pan_frames(3, h0, w0, step=2)


_full_expected = {}


def full_expected(oracle, weights, h0, w0, finish, sigma, protect):
    key = (h0, w0, finish, sigma, protect)
    if key not in _full_expected:
        f0 = full_frames(h0, w0)
        m0 = region_ref.mask("ramp", h0, w0)
        _full_expected[key] = sr.fullres_sequence(oracle, f0, [m0] * 3, synth.image(*REF0), *weights, MAX_SIDE, finish, sigma, kinds=FULL_KINDS, mot=MOT, levels=2, protect=protect)
    return _full_expected[key]


@pytest.mark.parametrize("h0,w0,finish,sigma", [(112, 128, nct.FINISH_EXACT, None), (112, 128, nct.FINISH_UPSAMPLE, None), (112, 128, nct.FINISH_UPSAMPLE, 10.0),
                                                (90, 131, nct.FINISH_UPSAMPLE, None)])
def test_fullres_masked_sequence(wctx, oracle, weights, h0, w0, finish, sigma):
    """a full frame, a blended one and a propagated one with the mask at the original size, against the composition; the state is the working-size sequence's"""
    protect = 1 if sigma else 0
    exp, keeps, _ = full_expected(oracle, weights, h0, w0, finish, sigma, protect)
    f0 = full_frames(h0, w0)
    m0 = region_ref.mask("ramp", h0, w0)
    wctx.set_finish_guided(sigma)
    try:
        wctx.seq_begin_fullres(synth.image(*REF0), f0[0].shape, MAX_SIDE, finish, _params(2))
        try:
            wctx.seq_set_motion(*MOT)
            wctx.seq_set_region(m0, protect)
            for t, k in enumerate(FULL_KINDS):
                out, lv = wctx.seq_frame_propagate_region_levels(f0[t]) if k == "P" else wctx.seq_frame_region_levels(f0[t])
                assert out.shape == f0[t].shape
                for l in range(2):
                    assert np.array_equal(words(lv["ab_blend"][l]), words(keeps[t]["ab_blend"][l])), ("ab_blend", t, l)
                top_mix = keeps[t]["ab_mix"] if k == "P" else keeps[t]["ab_mix"][1]
                assert np.array_equal(words(lv["ab_mix"][1]), words(top_mix)), ("ab_mix", t)
                assert np.array_equal(out, exp[t]), (t, k, int((out != exp[t]).any(axis=-1).sum()))
                assert not np.array_equal(out, f0[t])
        finally:
            wctx.seq_end()
    finally:
        wctx.set_finish_guided(None)


@pytest.mark.parametrize("finish,sigma", [(nct.FINISH_EXACT, None), (nct.FINISH_UPSAMPLE, None), (nct.FINISH_UPSAMPLE, 10.0)])
def test_fullres_identities_b_c_d(wctx, finish, sigma):
    """(b), (c) and (d) through every finish: M0 = 255 is the unmasked full-resolution sequence, M0 = 0 returns the original frames, and with the exact finish the first
    frame is nct_process_pair_fullres_region"""
    f0 = full_frames(112, 128)
    ref0 = synth.image(*REF0)
    prm = _params(2)

    def run(mask0, protect=0):
        wctx.seq_begin_fullres(ref0, f0[0].shape, MAX_SIDE, finish, prm)
        try:
            wctx.seq_set_motion(*MOT)
            if mask0 is not None:
                wctx.seq_set_region(mask0, protect)
            return [wctx.seq_frame_propagate(f) if k == "P" else wctx.seq_frame(f) for f, k in zip(f0, FULL_KINDS)]
        finally:
            wctx.seq_end()
    wctx.set_finish_guided(sigma)
    try:
        plain = run(None)
        for protect in (0, 1):
            assert all(np.array_equal(a, b) for a, b in zip(run(region_ref.mask("full", 112, 128), protect), plain)), ("b", protect)
            assert all(np.array_equal(a, b) for a, b in zip(run(region_ref.mask("empty", 112, 128), protect), f0)), ("c", protect)
        if finish == nct.FINISH_EXACT:
            m0 = region_ref.mask("half", 112, 128)
            assert np.array_equal(run(m0, 1)[0], wctx.process_pair_fullres_region(f0[0], m0, ref0, MAX_SIDE, 1, prm))
    finally:
        wctx.set_finish_guided(None)


# ---- test 5: nct_seq_frame_auto with a mask

@pytest.mark.parametrize("clip", ["pan", "cut"])
def test_auto_with_a_mask(wctx, ref, clip):
    """(f): the decisions and the probe's record are the unmasked sequence's; the bytes are those of the manual calls the decisions name; a CUT frame is the masked pair"""
    fr, mot, auto = ar.clips(H, W)[clip]
    au = nct.seq_auto(*auto)
    m = region_ref.mask("half", H, W)
    prm = _params(3)                                                       # three levels: the probe measures at level 2, where the clips' plans are F P P K P and F P C P
    strip = lambda d: {k: v for k, v in d.items() if k != "probe_ms"}

    def walk(mask):
        begin(wctx, ref, 3, motion=False)
        try:
            wctx.seq_set_motion(*mot)
            if mask is not None:
                wctx.seq_set_region(mask)
            outs, ds, probes = [], [], []
            for t, f in enumerate(fr):
                if t > 0:
                    probes.append(strip(wctx.seq_probe(f, au)))
                o, d = wctx.seq_frame_auto(f, au)
                outs.append(o); ds.append(strip(d))
            wctx.seq_reset()
            manual = []
            for f, d in zip(fr, ds):
                if d["kind"] == ar.SCENE_CUT:
                    wctx.seq_reset()
                manual.append(wctx.seq_frame_propagate(f) if d["kind"] == ar.PROPAGATED else wctx.seq_frame(f))
            return outs, ds, probes, manual
        finally:
            wctx.seq_end()
    plain_outs, plain_ds, plain_probes, _ = walk(None)
    outs, ds, probes, manual = walk(m)
    kinds = ar.kinds(plain_ds)
    assert kinds == {"pan": "FPPKP", "cut": "FPCP"}[clip]                  # the clips hold what they are here for
    assert ds == plain_ds and probes == plain_probes
    assert all(np.array_equal(a, b) for a, b in zip(outs, manual))
    assert not any(np.array_equal(a, b) for a, b in zip(outs, plain_outs))
    if clip == "cut":
        t = kinds.index("C")
        assert np.array_equal(outs[t], wctx.process_pair_region(fr[t], m, ref, 0, prm))


# ---- test 6: nct_pair_fit_lut after a masked frame

def test_pair_fit_lut_after_a_masked_frame(wctx, frames, ref):
    m = region_ref.mask("half", H, W)
    begin(wctx, ref, 2)
    try:
        wctx.seq_set_region(m)
        out = wctx.seq_frame(frames[0])
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit_masked(frames[0], out, m, 9))
        out = wctx.seq_frame_propagate(frames[1])
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit_masked(frames[1], out, m, 9))
        assert not np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit(frames[1], out, 9))
    finally:
        wctx.seq_end()
    f0 = full_frames(112, 128)
    m0 = region_ref.mask("half", 112, 128)
    wctx.seq_begin_fullres(synth.image(*REF0), f0[0].shape, MAX_SIDE, nct.FINISH_UPSAMPLE, _params(2))
    try:
        wctx.seq_set_region(m0)
        out = wctx.seq_frame(f0[0])
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit_masked(f0[0], out, m0, 9))
        out = wctx.seq_frame_propagate(f0[1])
        assert np.array_equal(wctx.pair_fit_lut(9), wctx.lut_fit_masked(f0[1], out, m0, 9))
    finally:
        wctx.seq_end()


# ---- test 7: refusals and state

def refused(call, code, word):
    with pytest.raises(nct.NctError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals_and_the_life_of_the_mask(wctx, frames, ref):
    m, ramp = region_ref.mask("half", H, W), region_ref.mask("ramp", H, W)
    refused(lambda: wctx.seq_set_region(m), -5, "no sequence is open")
    plain = [o for o, _ in unmasked(wctx, frames[:2], ref, 2, motion=False)]
    begin(wctx, ref, 2, motion=False)
    try:
        refused(lambda: wctx.seq_set_region(m[:-1]), -2, "mask")
        refused(lambda: wctx.seq_frame_region_levels(frames[0], want_color=False), -5, "no region mask is set")
        refused(lambda: wctx._chk(wctx._l.nct_pair_set_region(wctx._h, m.ctypes.data, None)), -5, "sequence is open")      # the pair's setter keeps its refusal
        wctx.seq_set_region(m, 1)
        for protect in (-1, 2):
            refused(lambda: wctx.seq_set_region(ramp, protect), -2, "protect")
        a0 = wctx.seq_frame(frames[0])                                                         # the previous setting still acts: mask `m`, protect 1
        a1 = wctx.seq_frame(frames[1])
        wctx.seq_reset()                                                                       # the mask survives a reset
        assert np.array_equal(wctx.seq_frame(frames[0]), a0) and np.array_equal(wctx.seq_frame(frames[1]), a1)
        assert not np.array_equal(a0, plain[0])
        wctx.seq_set_region(None)                                                              # NULL removes it: the next frames are the unmasked sequence's
        refused(lambda: wctx.seq_frame_propagate_region_levels(frames[1]), -5, "no region mask is set")
        wctx.seq_reset()
        assert np.array_equal(wctx.seq_frame(frames[0]), plain[0]) and np.array_equal(wctx.seq_frame(frames[1]), plain[1])
        wctx.seq_set_region(m, 1)
    finally:
        wctx.seq_end()
    expect_a0 = wctx.process_pair_region(frames[0], m, ref, 1, _params(2))
    assert np.array_equal(a0, expect_a0)
    # gone after nct_seq_end: a new sequence is unmasked
    again = [o for o, _ in unmasked(wctx, frames[:2], ref, 2, motion=False)]
    assert all(np.array_equal(a, b) for a, b in zip(again, plain))
