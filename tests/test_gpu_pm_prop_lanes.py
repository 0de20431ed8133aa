"""k_pm_prop lists a wave's propagation candidates with one lane per (query slot, neighbour) and scans them with one lane per slot. These are the smallest maps on which
that front end can go wrong, through the existing seams (pm_bench_setup / pm_bench_run_bidir / pm_bench_run) against the CPU oracle. Bars as in
test_patchmatch_bidir_bit_exact: identical NNFs, bit-identical distances in both directions, pm_mode 0 and 1 with equal evaluation and acceptance counters.
Workgroup tiles: 8x8 queries at C = 64, 8x4 at C = 128, 4x4 at C = 256 / 512."""
import functools

import numpy as np
import pytest
import synth

pytestmark = pytest.mark.gpu

SEED = 77


def two_colour(seed, C, H, W):
    """A map of only two feature vectors in 3x2 blocks: most distances tie, and the neighbours of a query often hold the same match, so that several of them
    propose the same candidate (listed, evaluated and counted once per proposer)."""
    rng = np.random.default_rng(seed)
    v = rng.random((2, C), dtype=np.float32) + np.float32(0.1)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(v[((yy // 3) + (xx // 2)) % 2].transpose(2, 0, 1))


def dead(seed, C, H, W):
    f = synth.features(seed, C, H, W)
    f[:, 1:3, 2:5] = 0; f[:, H - 1, W - 1] = 0; f[:, H // 2, 0] = 0
    return f


MAKERS = {"smooth": synth.features, "two_colour": two_colour, "dead": dead}


@functools.lru_cache(maxsize=None)
def reference(kind, C, ah, aw, bh, bw, iters, rs):
    """(raw fa, raw fb, oracle ann, annd, bnn, bnnd): computed once per case and shared; callers do not write to it."""
    import oracle_bind
    orc = oracle_bind.load()
    fa, fb = MAKERS[kind](21, C, ah, aw), MAKERS[kind](22, C, bh, bw)
    a, b = orc.feat_normalize(fa), orc.feat_normalize(fb)
    ann, annd = orc.patchmatch(a, b, orc.nnf_init(ah, aw, bh, bw), iters=iters, rs_max=rs, seed=SEED)
    bnn, bnnd = orc.patchmatch(b, a, orc.nnf_init(bh, bw, ah, aw), iters=iters, rs_max=rs, seed=SEED ^ 0x5bd1e995)
    return fa, fb, ann, annd, bnn, bnnd


def same_or_both_nan(a, b):
    """bit-identical where finite, NaN where the other is NaN (the payload of 0/0 differs between x86 and gfx950), as in test_patchmatch_dead_feature_pixels"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def check_bidir(ctx, kind, C, ah, aw, bh, bw, iters, rs):
    fa, fb, o_ann, o_annd, o_bnn, o_bnnd = reference(kind, C, ah, aw, bh, bw, iters, rs)
    ctx.pm_bench_setup(fa, fb)
    counts = []
    for mode in (0, 1):
        _, cnt, ann, annd, bnn, bnnd = ctx.pm_bench_run_bidir(iters=iters, rs_max=rs, seed=SEED, pm_mode=mode, count=True, fetch=True, both=True)
        assert np.array_equal(ann, o_ann) and np.array_equal(bnn, o_bnn), f"mode {mode}: NNF differs from the oracle"
        if kind == "dead":
            assert same_or_both_nan(annd, o_annd) and same_or_both_nan(bnnd, o_bnnd), f"mode {mode}: distances differ"
        else:
            assert np.array_equal(annd.view(np.uint32), o_annd.view(np.uint32)) and np.array_equal(bnnd.view(np.uint32), o_bnnd.view(np.uint32)), f"mode {mode}: distances differ"
        counts.append(cnt)
    assert counts[0] == counts[1] and counts[0][0] > 0, counts         # same candidates, same acceptances
    return counts[0]


CASES = [
    # kind, C, ah, aw, bh, bw, iters, rs_max
    # tiles partly inside the image on both axes, a last tile with one live row / column
    ("smooth", 64, 9, 17, 17, 9, 5, 8),
    ("smooth", 128, 9, 5, 6, 11, 5, 8),
    ("smooth", 256, 5, 6, 7, 5, 5, 4),
    ("smooth", 512, 5, 6, 7, 5, 5, 4),
    # narrower than every propagation jump (two pixels, the smallest side an NNF takes): each neighbour at +-8 / 4 / 2 across the narrow axis lies outside
    ("smooth", 64, 2, 19, 18, 2, 5, 8),
    ("smooth", 128, 2, 9, 10, 2, 5, 4),
    ("smooth", 256, 2, 2, 3, 5, 5, 4),
    ("smooth", 512, 2, 7, 6, 2, 5, 4),
    # exactly one tile wide (and, for the other direction, exactly one tile high)
    ("smooth", 64, 19, 8, 8, 21, 5, 8),
    ("smooth", 128, 9, 8, 4, 13, 5, 8),
    ("smooth", 256, 9, 4, 4, 7, 5, 4),
    ("smooth", 512, 4, 4, 4, 8, 5, 4),
    # 4 * iters > 250: no stamps (tstep = 0 throughout, every step strips)
    ("smooth", 64, 12, 10, 10, 12, 63, 4),
    ("smooth", 128, 12, 10, 10, 12, 63, 4),
    # dead (all-zero -> NaN) feature pixels
    ("dead", 64, 13, 17, 11, 19, 5, 8),
    ("dead", 256, 9, 10, 11, 7, 5, 4),
    # several neighbours propose the same candidate
    ("two_colour", 64, 20, 23, 18, 25, 5, 8),
    ("two_colour", 128, 11, 14, 13, 9, 5, 8),
    ("two_colour", 256, 9, 11, 10, 7, 5, 4),
]


@pytest.mark.parametrize("kind,C,ah,aw,bh,bw,iters,rs", CASES)
def test_pm_prop_lanes_bidir_bit_exact(ctx, kind, C, ah, aw, bh, bw, iters, rs):
    check_bidir(ctx, kind, C, ah, aw, bh, bw, iters, rs)


@pytest.mark.parametrize("C,ah,aw,bh,bw", [(64, 37, 41, 33, 45), (128, 21, 26, 19, 23)])
def test_pm_prop_lanes_stale_candidates_are_skipped(ctx, C, ah, aw, bh, bw):
    """From the fifth step on a neighbour whose match has not changed for four steps proposes nothing: four iterations evaluate fewer candidates than four times
    the first one (both runs also checked bit for bit)."""
    four = check_bidir(ctx, "smooth", C, ah, aw, bh, bw, 4, 8)
    one = check_bidir(ctx, "smooth", C, ah, aw, bh, bw, 1, 8)
    assert four[0] < 4 * one[0], (four, one)


@pytest.mark.parametrize("C,ah,aw,bh,bw", [(64, 9, 17, 17, 9), (128, 9, 5, 6, 11), (512, 5, 6, 7, 5)])
def test_pm_prop_lanes_single_direction(ctx, C, ah, aw, bh, bw):
    """pm_bench_run: the second job of every launch is empty, plain evaluation."""
    fa, fb, o_ann, o_annd, _, _ = reference("smooth", C, ah, aw, bh, bw, 5, 8)
    ctx.pm_bench_setup(fa, fb)
    _, evals, nnf, dist = ctx.pm_bench_run(iters=5, rs_max=8, seed=SEED, count_evals=True, fetch=True)
    assert np.array_equal(nnf, o_ann)
    assert np.array_equal(dist.view(np.uint32), o_annd.view(np.uint32))
    assert evals > 0
