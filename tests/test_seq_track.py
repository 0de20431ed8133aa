"""Region tracking (SPEC §6.14) without a GPU: the identities of the numpy rule (tests/seq_track_ref.py) and the pan condition — on a clip that pans 4 px per frame the
matte carried through the fields of seq_mc_ref's search, found on the oracle's Lab pyramid, overlaps the truly shifted matte more than the static matte does. The
binding's surface is checked too: the three calls exist. Every comparison of mattes is equality of bytes."""
import numpy as np
import pytest

import nct
import seq_mc_ref
import seq_prop_ref
import seq_ref
import seq_track_ref as tr

MOT = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)


def test_binding_has_the_calls():
    for name in ("nct_seq_matte_warp", "nct_seq_matte_warp_dev", "nct_seq_set_region_tracking", "nct_seq_get_region"):
        assert name in nct.SIGNATURES and hasattr(nct.lib(), name), name
    for name in ("seq_matte_warp", "seq_set_region_tracking", "seq_get_region"):
        assert callable(getattr(nct.Context, name)), name


@pytest.mark.parametrize("case", range(len(tr.SEAM_CASES)))
def test_zero_field_keeps_the_input(case):
    mask, field = tr.seam_inputs(case, "zero")
    assert np.array_equal(tr.matte_warp(mask, field), mask)


@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (6, 1), (9, 11), (37, 70)])
@pytest.mark.parametrize("kind", ["random", "outside"])
def test_equal_sizes_are_the_gather_of_the_warp(grid, kind):
    """H == h, W == w: d = m, and the bytes are those seq_prop_ref.warp gathers (the matte carried as the words of a coefficient map)"""
    h, w = grid
    _, field = seq_prop_ref.warp_case(h, w, 5, kind)
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dy, dx = tr.displacement(field, h, w)
    assert np.array_equal(dy, field[..., 0].astype(np.int64)) and np.array_equal(dx, field[..., 1].astype(np.int64))
    as_map = np.repeat(mask.reshape(1, h * w, 1).astype(np.float64), 2, axis=0).repeat(3, axis=2)
    exp = seq_prop_ref.warp(as_map, field)[0, :, 0].reshape(h, w).astype(np.uint8)
    assert np.array_equal(tr.matte_warp(mask, field), exp)


def test_constant_field_scales_with_the_ratio():
    """(1, -2) on 9 x 11 carried to 36 x 44 is (4, -8) at every target pixel"""
    field = np.empty((9, 11, 2), np.int16); field[..., 0] = 1; field[..., 1] = -2
    dy, dx = tr.displacement(field, 36, 44)
    assert (dy == 4).all() and (dx == -8).all()
    mask = np.random.default_rng(1).integers(0, 256, (36, 44), dtype=np.uint8)
    yy, xx = np.mgrid[0:36, 0:44]
    assert np.array_equal(tr.matte_warp(mask, field), mask[np.clip(yy + 4, 0, 35), np.clip(xx - 8, 0, 43)])


def test_a_byte_is_copied_never_interpolated():
    """a binary matte stays binary and all-255 stays all-255 under any field, the non-integer ratio and the extremes included"""
    for case in range(len(tr.SEAM_CASES)):
        for kind in tr.FIELD_KINDS:
            mask, field = tr.seam_inputs(case, kind)
            binary = np.where(mask >= 128, 255, 0).astype(np.uint8)
            assert set(np.unique(tr.matte_warp(binary, field))) <= {0, 255}
            assert (tr.matte_warp(np.full_like(mask, 255), field) == 255).all()


def test_axis_rule_matches_the_float_index_rule():
    """the exact fraction is cv::resize's centre-aligned index: s + t / D == (x + 0.5) * n / N - 0.5 wherever no clamp acts"""
    for N, n in ((56, 14), (45, 17), (131, 7), (34, 33), (9, 9)):
        s, s1, t, D = tr.axis(N, n)
        f = (np.arange(N) + 0.5) * n / N - 0.5
        free = (f >= 0) & (np.floor(f) < n - 1)
        assert np.allclose((s + t / D)[free], f[free], rtol=0, atol=1e-12)
        assert (s >= 0).all() and (s1 <= n - 1).all() and (t >= 0).all() and (t < D).all()


def test_pan_condition(oracle):
    """six frames of a 4 px pan, a rectangle matte on frame 0: after five carries through the top level's fields the matte is closer to the truly shifted matte than the
    matte that stayed. Measured: IoU 1.0000 carried, 0.1667 static, with the field of the 56 x 64 level and with the 14 x 16 level's alike"""
    H, W, step = 56, 64, 4
    frames = seq_ref.pan_frames(6, H, W, step=step)
    m0 = tr.rect(H, W, 16, 40, 30, 58)
    truth = tr.shifted(m0, 5 * step)
    static = tr.iou(m0, truth)
    for levels in (5, 3):
        M, ages = tr.carried(oracle, frames, [m0] + [None] * 5, MOT, levels)
        assert ages == [0, 1, 2, 3, 4, 5]
        got = tr.iou(M[5], truth)
        print("levels %d: IoU carried %.4f, static %.4f" % (levels, got, static))
        assert got > static, (levels, got, static)
        assert set(np.unique(M[5])) <= {0, 255}
    # motion off: the matte stays, the age counts
    M, ages = tr.carried(oracle, frames, [m0] + [None] * 5, None, 5)
    assert all(np.array_equal(m, m0) for m in M) and ages == [0, 1, 2, 3, 4, 5]
