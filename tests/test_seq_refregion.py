"""Reference region masks in sequences (SPEC §6.19) without a GPU: the numpy rule of the held pull (tests/seq_refregion_ref.py) against the scalar loop, its limits,
the composition's identities (b), (c) and (d) against seq_multi_ref.sequence / refregion_ref.run, and the quality figure: on a static noisy scene the held pull changes
no more from frame to frame than the free one."""
import numpy as np
import pytest

import refregion_ref
import region_ref
import seq_multi_ref
import seq_ref
import seq_refregion_ref as srr
import synth

FRAME, REF = (40, 36), (34, 38)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (6, 1), (9, 11)])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("field", [None, "zero", "random", "extreme"])
def test_numpy_rule_matches_the_scalar_loop(grid, K, field):
    h, w = grid
    for with_mask in (True, False):
        c = srr.hold_case(h, w, K, 100 * K + 7 * h + w, field, with_mask, unmasked=1 if K > 1 else None)
        for tau in (0.0, 0.7, 1.0 - 2.0 ** -53):
            for sigma in (10.0, 0.75):
                got = srr.pull_hold(*srr.args_of(c), tau, sigma)
                exp = srr.pull_hold_scalar(*srr.args_of(c), tau, sigma)
                for g, e, name in zip(got, exp, ("held", "mask", "free")):
                    assert g.dtype == np.uint8 and np.array_equal(g, e), (name, with_mask, tau, sigma)


def test_limits_of_the_hold():
    c = srr.hold_case(9, 11, 2, 5, "random", True, unmasked=1)
    held, M, P = srr.pull_hold(*srr.args_of(c), 0.0, 10.0)
    assert np.array_equal(held, P) and np.array_equal(M, np.minimum(P, c["src_mask"]))         # tau = 0: the free pull
    assert np.array_equal(P, refregion_ref.merge(c["label"], c["pulled"])) and (P[c["label"] == 1] == 255).all()
    # the held byte lies between the free one and the kept one along the motion
    held, _, _ = srr.pull_hold(*srr.args_of(c), 0.7, 10.0)
    j = seq_multi_ref.carry(c["prev"], c["field"])
    assert ((held >= np.minimum(P, j)) & (held <= np.maximum(P, j))).all() and not np.array_equal(held, P)
    # every map 255: exactly 255, whatever the weight (identity (b)); every map 0 and a kept 0: exactly 0
    full = np.full((9, 11), 255, np.uint8)
    assert (srr.pull_hold([full, None], c["label"], full, c["lab"], c["lab_prev"], c["field"], None, 0.7, 10.0)[0] == 255).all()
    zero = np.zeros((9, 11), np.uint8)
    assert not srr.pull_hold([zero], None, zero, c["lab"], c["lab_prev"], c["field"], None, 0.7, 10.0)[0].any()
    # the weight is the blend's: on equal Lab maps with no field tau_p = tau everywhere
    held, _, P = srr.pull_hold(c["pulled"], c["label"], c["prev"], c["lab"], c["lab"], None, None, 0.5, 10.0)
    assert np.array_equal(held, np.rint(P + 0.5 * (c["prev"].astype(np.float64) - P)).astype(np.uint8))


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


@pytest.fixture(scope="module")
def fixture():
    frames = seq_ref.pan_frames(4, FRAME[0], FRAME[1], step=2)
    ref = synth.image(1001, REF[0], REF[1])
    return frames, ref, region_ref.mask("half", REF[0], REF[1])


def test_all_255_is_the_unmasked_sequence(oracle, weights, fixture):
    """identity (b): bytes and kept state on every frame kind, one and two references"""
    ws, bs = weights
    frames, ref, _ = fixture
    full = np.full(REF, 255, np.uint8)
    mot = (3, 1, 1)
    for refs in ([ref], [ref, seq_multi_ref.competing(ref)]):
        exp, ek = seq_multi_ref.sequence(oracle, frames, refs, ws, bs, mot=mot, levels=2, full=[k != "P" for k in srr.KINDS])
        got, gk, states = srr.sequence(oracle, frames, None, refs, [full] + [None] * (len(refs) - 1), ws, bs, mot=mot, levels=2)
        for t in range(4):
            assert np.array_equal(got[t], exp[t]), t
            for l in range(2):
                assert np.array_equal(bits(states[t][l][0]), bits(ek[t]["ab_blend"][l])), (t, l)
                assert (gk[t]["p_held"][l] == 255).all()
                assert np.array_equal(gk[t]["label"][l], ek[t]["label"][l])


def test_all_zero_is_the_source(oracle, weights, fixture):
    """identity (c): K = 1 and Q == 0 — every frame is its source, for either protect"""
    ws, bs = weights
    frames, ref, _ = fixture
    for protect in (0, 1):
        got, _, _ = srr.sequence(oracle, frames, None, [ref], [np.zeros(REF, np.uint8)], ws, bs, levels=2, protect=protect)
        assert all(np.array_equal(g, f) for g, f in zip(got, frames)), protect


def test_frames_without_a_blend_are_the_masked_run(oracle, weights, fixture):
    """identity (d): a first frame, a frame after a reset and every frame with tau == 0 equal refregion_ref.run"""
    ws, bs = weights
    frames, ref, q = fixture
    refs, qs = [ref, seq_multi_ref.competing(ref)], [q, None]
    exp = [refregion_ref.run(oracle, f, None, refs, qs, ws, bs, levels=2) for f in frames[:3]]
    got, gk, _ = srr.sequence(oracle, frames[:3], None, refs, qs, ws, bs, kinds="FBB", levels=2, reset_before=(2,))
    zero, zk, _ = srr.sequence(oracle, frames[:3], None, refs, qs, ws, bs, kinds="FBB", levels=2, tau=0.0)
    for t in (0, 2):
        assert np.array_equal(got[t], exp[t][0]), t
    assert not np.array_equal(got[1], exp[1][0])                                                # the blended frame is another one
    for t in range(3):
        assert np.array_equal(zero[t], exp[t][0]), t
        for l in range(2):
            assert np.array_equal(zk[t]["p_held"][l], exp[t][1]["p"][l]) and np.array_equal(zk[t]["mask_full"][l], exp[t][1]["mask_full"][l])
    # a mask replaced mid-sequence: that full frame keeps its free pull
    q2 = np.ascontiguousarray(q[:, ::-1])
    _, rk, _ = srr.sequence(oracle, frames[:2], None, [ref], [[q], [q2]], ws, bs, kinds="FB", levels=2)
    assert all(np.array_equal(rk[1]["p_held"][l], rk[1]["p_free"][l]) for l in range(2))
    _, hk, _ = srr.sequence(oracle, frames[:2], None, [ref], [q], ws, bs, kinds="FB", levels=2)
    assert any(not np.array_equal(hk[1]["p_held"][l], hk[1]["p_free"][l]) for l in range(2))      # where the mask stays, the same frame holds


def test_quality_figure(oracle, weights):
    """SPEC §6.19 / DESIGN §3.24: four noisy frames of a static scene, a half mask on the reference. The mean |P'_t - P'_(t-1)| on the last level run with the hold does
    not exceed the free pull's (tau = 0 for the mask only). Measured by this reference, not by the code under test; both figures are printed"""
    ws, bs = weights
    frames = seq_ref.static_frames(4, 56, 64)
    ref = synth.image(1001, 48, 60)
    q = region_ref.mask("half", 48, 60)
    held = srr.pull_flicker(srr.sequence(oracle, frames, None, [ref], [q], ws, bs, kinds="FBBB", levels=2)[1])
    free = srr.pull_flicker(srr.sequence(oracle, frames, None, [ref], [q], ws, bs, kinds="FBBB", levels=2, hold_pull=False)[1])
    print("mean |P'_t - P'_(t-1)| on the last level run: held %.3f, free %.3f" % (held, free))
    assert held <= free, (held, free)
