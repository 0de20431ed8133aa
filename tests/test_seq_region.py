"""Region masks in sequences (SPEC §6.13) without a GPU: the reference composition (tests/seq_region_ref.py) against itself — identities (b), (c), (d), (e) and (g)
of rule 5 on four frames of a pan with kinds F B P B and motion on, a mask that changes from frame to frame, and the numpy masked finish against the unfused chain.
Every comparison is equality of bytes or of bit patterns."""
import numpy as np
import pytest

import region_ref
import seq_mc_ref
import seq_ref
import seq_region_ref as sr
import synth

H, W = 56, 64
REF = (2000, 48, 60)
MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)


def words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def clip():
    return seq_ref.pan_frames(4, H, W), synth.image(*REF)


def changing_masks():
    return [region_ref.mask(k, H, W) for k in ("half", "ramp", "random", "half")]


_runs = {}


def run(oracle, weights, clip, levels, which):
    """one sequence of the plan per (levels, masks), computed once: "none" (the unmasked sequence), "full" (M = 255), "empty" (M = 0), "changing" """
    key = (levels, which)
    if key not in _runs:
        frames, ref = clip
        masks = {"none": [None] * 4, "full": [region_ref.mask("full", H, W)] * 4, "empty": [region_ref.mask("empty", H, W)] * 4, "changing": changing_masks()}[which]
        _runs[key] = sr.sequence(oracle, frames, masks, ref, *weights, kinds=sr.KINDS, mot=MOT, levels=levels)
    return _runs[key]


@pytest.mark.parametrize("levels", [5, 2])
def test_full_mask_is_the_unmasked_sequence(oracle, weights, clip, levels):
    """(b): M = 255 — every frame's bytes and every level's kept state are the unmasked sequence's; the mixed map is the state, word for word"""
    outs, keeps, states = run(oracle, weights, clip, levels, "full")
    uouts, ukeeps, ustates = run(oracle, weights, clip, levels, "none")
    for t, kind in enumerate(sr.KINDS):
        assert np.array_equal(outs[t], uouts[t]), (t, kind)
        for l in range(levels):
            assert np.array_equal(words(states[t][l][0]), words(ustates[t][l][0])), (t, l)
            assert np.array_equal(states[t][l][1], ustates[t][l][1]), (t, l)
        if kind == "P":
            assert np.array_equal(words(keeps[t]["ab_mix"]), words(states[t][levels - 1][0]))
        else:
            assert all(np.array_equal(words(keeps[t]["ab_mix"][l]), words(keeps[t]["ab_blend"][l])) for l in range(levels))
    if levels == 5:                                            # the pan moves a pixel per frame: the fine levels find a field, the blend and the warp are at work
        assert any(m.any() for m in keeps[1]["motion"]) and any(m.any() for m in keeps[2]["motion"])


@pytest.mark.parametrize("levels", [5, 2])
def test_empty_mask_returns_every_source(oracle, weights, clip, levels):
    """(c): M = 0 — every frame kind returns its source byte for byte, and the state it keeps is still a transfer (not the identity)"""
    outs, keeps, states = run(oracle, weights, clip, levels, "empty")
    frames, _ = clip
    for t, kind in enumerate(sr.KINDS):
        assert np.array_equal(outs[t], frames[t]), (t, kind)
        x = states[t][levels - 1][0]
        assert not (np.array_equal(x[0], np.ones_like(x[0])) and not x[1].any())


@pytest.mark.parametrize("levels", [5, 2])
def test_level0_state_does_not_depend_on_the_mask(oracle, weights, clip, levels):
    """(e): level 0 sees features of the source alone, so its kept X' is the unmasked sequence's word for word on every frame — under M = 0 and under a mask that changes
    from frame to frame alike: on frame t the sequence is where the same sequence run with frame t's mask from the start would be"""
    _, _, ustates = run(oracle, weights, clip, levels, "none")
    for which in ("empty", "changing"):
        _, keeps, states = run(oracle, weights, clip, levels, which)
        for t in range(4):
            assert np.array_equal(words(states[t][0][0]), words(ustates[t][0][0])), (which, t)
            assert np.array_equal(states[t][0][1], ustates[t][0][1]), (which, t)
    # the finer levels see the composed result: there the masked sequence is another sequence (the comparison above is not vacuous)
    _, _, states = run(oracle, weights, clip, levels, "empty")
    assert not np.array_equal(words(states[0][levels - 1][0]), words(ustates[0][levels - 1][0]))


@pytest.mark.parametrize("levels", [5, 2])
def test_first_frame_and_tau0_equal_the_masked_pair(oracle, weights, clip, levels):
    """(d): the first frame is region_ref.pair(S_0, M_0, R); so is every frame with tau == 0"""
    frames, ref = clip
    masks = changing_masks()
    outs, keeps, _ = run(oracle, weights, clip, levels, "changing")
    exp0, pk = region_ref.pair(oracle, frames[0], masks[0], ref, *weights, levels=levels)
    assert np.array_equal(outs[0], exp0)
    assert all(np.array_equal(words(keeps[0]["ab_mix"][l]), words(pk["ab_mix"][l])) for l in range(levels))
    assert not np.array_equal(outs[1], region_ref.pair(oracle, frames[1], masks[1], ref, *weights, levels=levels)[0])      # a blended frame is another picture
    if levels == 2:
        o, _, _ = sr.sequence(oracle, frames[:2], masks[:2], ref, *weights, kinds="FB", tau=0.0, mot=MOT, levels=levels)
        assert np.array_equal(o[0], exp0)
        assert np.array_equal(o[1], region_ref.pair(oracle, frames[1], masks[1], ref, *weights, levels=levels)[0])


@pytest.mark.parametrize("levels", [5, 2])
def test_identical_frame_with_the_same_mask_propagates_to_identical_output(oracle, weights, clip, levels):
    """(g)"""
    frames, ref = clip
    m = region_ref.mask("ramp", H, W)
    for protect in (0, 1):
        outs, keeps, _ = sr.sequence(oracle, [frames[0], frames[0]], [m, m], ref, *weights, kinds="FP", mot=MOT, levels=levels, protect=protect)
        assert np.array_equal(outs[1], outs[0]), protect
        assert not any(f.any() for f in keeps[1]["motion"])
        assert not np.array_equal(outs[0], frames[0])


@pytest.mark.parametrize("case", range(len(sr.SEAM_CASES)))
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("protect", [0, 1])
def test_numpy_masked_finish_equals_the_unfused_chain(oracle, case, guided, protect):
    """rule 4: the masked upsampling finish is the upsampling (guided) finish's Lab_o composed by §6.11 rule 3 — and its inputs reach every outcome"""
    import finish_guided_ref
    import finish_up_ref
    ab, lab_w, h, w, s_full, mask = sr.seam_inputs(oracle, case)
    for form in (0, 1):
        got, olab = sr.masked_finish(oracle, ab, h, w, s_full, mask, protect, form, lab_w if guided else None)
        if guided:
            _, lab_o = finish_guided_ref.finish_guided(oracle, ab, lab_w, h, w, s_full, finish_guided_ref.SIGMA, form)
        else:
            _, lab_o = finish_up_ref.oracle_finish_upsample(oracle, ab, h, w, s_full, form)
        assert np.array_equal(olab, lab_o)
        assert np.array_equal(got, region_ref.compose(oracle, s_full, lab_o, mask, protect, form))
    by_protect, unmoved, converted = sr.outcome_shares(oracle, olab, s_full, mask, protect)
    shares = region_ref.compose_shares(oracle.bgr2lab(s_full), olab, mask)
    assert shares[1] > 0 and unmoved > 0 and converted > 0 and (mask == 0).any()
    if protect:
        assert by_protect > 0
    # M = 255 everywhere: the unmasked finish
    full = np.full(mask.shape, 255, np.uint8)
    assert np.array_equal(sr.masked_finish(oracle, ab, h, w, s_full, full, protect, 0, lab_w if guided else None)[0], oracle.lab2bgr(olab, 0))
