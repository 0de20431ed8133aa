"""Frame sequences over several references (SPEC §6.18) without a GPU: the numpy rule of the held selection (tests/seq_multi_ref.py) against the scalar loop in the
canonical order, its limits (hold = 0 on distinct scores, hold = 2, one reference, a stale kept label), the label carry, the composition's identities, and the quality
statement on the two fixtures: the default hold flips fewer labels along the motion than the free selection, and hold = 2 none on the static scene."""
import numpy as np
import pytest

import multi_ref
import seq_mc_ref
import seq_multi_ref as smr
import seq_ref

GRIDS = [(1, 1), (1, 7), (3, 3), (7, 5)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", smr.KINDS)
def test_numpy_rule_matches_the_scalar_loop(grid, K, kind):
    h, w = grid
    for with_field in (True, False):
        c = smr.hold_case(h, w, K, 1000 * K + 31 * h + w, kind, with_field)
        for hold in (0.0, 0.02, 2.0):
            for sigma in (10.0, 0.75):
                args = (c["errs"], c["prev_label"], c["lab"], c["lab_prev"], c["field"], hold, sigma)
                lab, free, margin = smr.select_hold(*args)
                elab, efree, emargin = smr.select_hold_scalar(*args)
                assert lab.dtype == np.uint8 and np.array_equal(lab, elab), (with_field, hold, sigma)
                assert np.array_equal(free, efree) and np.array_equal(bits(margin), bits(emargin))
                assert np.array_equal(free, multi_ref.select(c["errs"]))                    # f is §6.2 rule 2's label
                assert (lab < K).all()
                stale = smr.carry(c["prev_label"], c["field"]) >= K
                assert np.array_equal(lab[stale], free[stale])                               # a kept label >= K is never kept


def test_limits_of_hold():
    c = smr.hold_case(7, 5, 3, 5, "random")
    kept = smr.carry(c["prev_label"], c["field"])
    # hold = 2: E >= -1 per tap bounds a score difference by 2 n only where g = 1; on equal Lab maps g = 1 everywhere and nothing switches
    lab, free, margin = smr.select_hold(c["errs"], c["prev_label"], c["lab"], c["lab"], None, 2.0, 10.0)
    assert np.array_equal(lab, c["prev_label"]) and not np.array_equal(free, c["prev_label"])
    assert np.array_equal(bits(margin), bits(2.0 * smr.scores(c["errs"])[1].astype(np.float64)))
    # hold = 0: the margin is 0.0 and a kept label stays only on an exact tie of the two scores
    lab, free, margin = smr.select_hold(c["errs"], c["prev_label"], c["lab"], c["lab_prev"], c["field"], 0.0, 10.0)
    sc, _ = smr.scores(c["errs"])
    tie = np.take_along_axis(sc, kept.astype(np.int64)[None], axis=0)[0] == sc.min(axis=0)
    assert not margin.any() and np.array_equal(lab, np.where(tie, kept, free))
    # ties: every map the same -> f = 0, and any kept label stays for any hold
    t = smr.hold_case(7, 5, 3, 6, "ties")
    for hold in (0.0, 0.02):
        lab, free, _ = smr.select_hold(t["errs"], t["prev_label"], t["lab"], t["lab_prev"], t["field"], hold, 10.0)
        assert not free.any() and np.array_equal(lab, smr.carry(t["prev_label"], t["field"]))
    # where the frame changed the margin falls toward 0: with Lab maps 255 apart g = 1 / (1 + 65025 / sigma^2)
    far = np.zeros_like(c["lab"]); near = np.full_like(c["lab"], 255)
    _, _, margin = smr.select_hold(c["errs"], c["prev_label"], far, near, None, 2.0, 10.0)
    assert margin.max() < 2.0 * 9 / 600.0


def test_label_carry():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 8, (7, 5), dtype=np.uint8)
    assert np.array_equal(smr.carry(lab, None), lab) and np.array_equal(smr.carry(lab, np.zeros((7, 5, 2), np.int16)), lab)
    f = np.zeros((7, 5, 2), np.int16); f[..., 1] = 2                                        # what frame t shows at x, frame t-1 showed at x + 2
    exp = lab[:, np.minimum(np.arange(5) + 2, 4)]
    assert np.array_equal(smr.carry(lab, f), exp)
    f[..., 0] = -30                                                                          # a vector that leaves the grid is clamped to it
    assert np.array_equal(smr.carry(lab, f), np.broadcast_to(exp[0], (7, 5)))


@pytest.fixture(scope="module")
def weights():
    from caffemodel_io import synthetic_vgg19
    return synthetic_vgg19(19)


def test_one_reference_is_the_single_reference_composition(oracle, weights):
    ws, bs = weights
    ref = smr.quality_references()[0]
    frames = seq_ref.pan_frames(2, 40, 36, step=2)
    exp, ek = seq_mc_ref.sequence(oracle, frames, ref, ws, bs, levels=2)
    got, gk = smr.sequence(oracle, frames, [ref], ws, bs, levels=2)
    for t in range(2):
        assert np.array_equal(got[t], exp[t])
        for l in range(2):
            assert np.array_equal(bits(gk[t]["ab_blend"][l]), bits(ek[t]["ab_blend"][l])) and np.array_equal(gk[t]["motion"][l], ek[t]["motion"][l])
            assert not gk[t]["label"][l].any()
    # a repeated reference: label 0 everywhere, the bytes of the single-reference sequence, with a hold and motion on
    twice, tk = smr.sequence(oracle, frames, [ref, ref], ws, bs, levels=2, hold=0.05)
    assert all(np.array_equal(a, b) for a, b in zip(twice, exp)) and not any(l.any() for k in tk for l in k["label"])


@pytest.fixture(scope="module")
def quality(oracle, weights):
    """per fixture and hold in (0 = the free selection, the default, 2): the keeps of a two-frame sequence over the two competing references"""
    ws, bs = weights
    refs = smr.quality_references()
    res = {}
    for kind in ("static", "pan"):
        frames = smr.quality_frames(kind)
        for hold in (0.0, smr.HOLD, 2.0):
            if kind == "pan" and hold == 2.0:
                continue
            res[kind, hold] = smr.sequence(oracle, frames, refs, ws, bs, hold=hold)[1]
    return res


def test_quality_statement(quality):
    """SPEC §6.18: with the default hold the share of finest-level labels that flip along the motion is strictly below the free selection's on both fixtures; with
    hold = 2 it is zero on the static one. The references compete: the free selection flips at least 5 % of the finest labels between consecutive frames"""
    for kind in ("static", "pan"):
        free = smr.flip_share(quality[kind, 0.0])
        held = smr.flip_share(quality[kind, smr.HOLD])
        print("%s: flip share along the motion, free selection %.4f, hold %.3g: %.4f" % (kind, free, smr.HOLD, held))
        assert free >= 0.05, (kind, free)
        shares = multi_ref.shares(quality[kind, 0.0][0]["label"][-1], 2)
        assert min(shares) > 0.05, shares                                                    # both references hold a share of the finest label map
        assert held < free, (kind, held, free)
    assert smr.flip_share(quality["static", 2.0]) == 0.0
