"""The numpy reference of the 16-bit table apply (tests/lut16_ref.py, SPEC §6.20) alone, no GPU: the two properties the SPEC states and the edges of the cast."""
import numpy as np
import pytest

import lut16_ref
import lut_ref


def axis_sweep(N, seed):
    """[3 * 65536, 3] uint16: every 16-bit value on each axis in turn, the other two axes random"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 65536, (3, 65536, 3)).astype(np.uint16)
    for a in range(3):
        px[a, :, a] = np.arange(65536, dtype=np.uint16)
    return px.reshape(-1, 3)


# both calls round the same real value x (the double sums differ from it by about 1e-12): nct_lut_apply to an integer, the 16-bit apply 257 x to an integer
CONSISTENCY_BOUND = 0.5 + 0.5 / 257 + 1e-9


@pytest.mark.parametrize("N", lut_ref.SIZES)
def test_the_identity_table_returns_every_input(N):
    px = axis_sweep(N, N)
    assert np.array_equal(lut16_ref.apply(lut_ref.identity(N), N, px), px)


@pytest.mark.parametrize("N", lut_ref.SIZES)
def test_the_weights_are_exact_and_sum_to_65535_cubed(N):
    px = axis_sweep(N, 100 + N)[::97]
    total = np.zeros(len(px), np.int64)
    (ib, fb), (ig, fg), (ir, fr) = (lut16_ref._axis(px[:, c], N) for c in range(3))
    for i, f in ((ib, fb), (ig, fg), (ir, fr)):
        assert i.min() >= 0 and i.max() <= N - 2 and f.min() >= 0 and f.max() <= 65535
    for db in (0, 1):
        for dg in (0, 1):
            for dr in (0, 1):
                w = (fb if db else 65535 - fb) * (fg if dg else 65535 - fg) * (fr if dr else 65535 - fr)
                assert w.max() < 1 << 48 and np.array_equal(w.astype(np.float64).astype(np.int64), w)
                total += w
    assert (total == lut16_ref.W3).all() and lut16_ref.W3 == 281462092005375


@pytest.mark.parametrize("N", [3, 17, 33])
def test_consistency_with_the_8_bit_apply(N):
    rng = np.random.default_rng(7 + N)
    u = rng.integers(0, 256, (200000, 3)).astype(np.uint8)
    t = (lut_ref.identity(N).astype(np.float64) + rng.normal(0.0, 6.0, (N ** 3, 3))).astype(np.float32)       # identity plus noise: leaves [0, 255] near the faces
    o8 = lut_ref.apply(t, N, u).astype(np.float64)
    o16 = lut16_ref.apply(t, N, u.astype(np.uint16) * 257).astype(np.float64)
    worst = np.abs(o16 / 257.0 - o8).max()
    print("N = %d: max |o16 / 257 - o8| = %.5f" % (N, worst))
    assert worst <= CONSISTENCY_BOUND


def test_both_clamps_are_reached():
    N = 9
    t = (np.random.default_rng(3).random((N, N, N, 3)) * 400.0 - 70.0).astype(np.float32)
    px = np.random.default_rng(4).integers(0, 65536, (20000, 3)).astype(np.uint16)
    out = lut16_ref.apply(t, N, px)
    assert out.min() == 0 and out.max() == 65535
    low, high = np.full((N, N, N, 3), -1.0, np.float32), np.full((N, N, N, 3), 255.5, np.float32)
    assert (lut16_ref.apply(low, N, px) == 0).all() and (lut16_ref.apply(high, N, px) == 65535).all()


def test_a_nan_entry_gives_zero():
    N = 5
    t = lut_ref.identity(N).reshape(N, N, N, 3).copy()
    t[2, 2, 2, 1] = np.nan
    px = np.array([[32768, 32768, 32768], [32000, 33000, 31000], [0, 0, 0], [65535, 65535, 65535]], np.uint16)
    out = lut16_ref.apply(t, N, px)
    assert out[0, 1] == 0 and out[1, 1] == 0                  # the node itself and a cell that touches it: channel 1 is NaN, which the cast turns into 0
    assert out[0, 0] == 32768 and out[0, 2] == 32768          # the other channels are the identity's
    assert np.array_equal(out[2:], px[2:])                    # the far corners are not: their cells do not touch the node
