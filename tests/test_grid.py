"""The arithmetic of the local colour grids (SPEC §6.22) in its numpy reference tests/grid_ref.py, without a GPU: the properties the SPEC states and the quality figures
of the two-gradings fixture. tests/test_gpu_grid.py holds the GPU against the same reference bit for bit."""
import numpy as np
import pytest

import grid_ref
import lut_ref

# both applies round the same real value x (the double sums differ from it by about 1e-12): the 8-bit apply to an integer, the 16-bit apply 257 x to an integer
CONSISTENCY_BOUND = 0.5 + 0.5 / 257 + 1e-9
# the largest normwise backward error |M x - b| / (|M| |x| + |b|) (infinity norms) of the reference's L D L^T over the nodes of FIXTURE_FITS, measured: see
# test_ldl_agrees_with_numpy_solve
LDL_BACKWARD_ERROR = 1.42e-16
FIXTURE_FITS = [(g, lam) for g in ((2, 2, 2), (8, 8, 8), (16, 16, 16)) for lam in (1.0 / 16.0, 16.0, 65536.0)]


@pytest.fixture(scope="module")
def two():
    S, O = grid_ref.two_gradings()
    for a in (S, O):
        a.setflags(write=False)
    return S, O


def mae(a, b):
    return float(np.abs(a.astype(np.int64) - b.astype(np.int64)).mean())


def all_values_16():
    rng = np.random.default_rng(16)
    px = np.stack([np.arange(65536), rng.permutation(65536), rng.permutation(65536)], axis=-1).astype(np.uint16)      # all 65536 values on each channel
    return px.reshape(128, 512, 3)


def test_equal_images_give_the_zero_grid_and_a_zero_grid_returns_every_input(two):
    S, _ = two
    X, sums, blurred = grid_ref.fit(S, S, 8, 8, 8, 16.0)
    assert not X.any() and not sums[:, 10:].any() and sums[:, grid_ref.COUNT].sum() == S.shape[0] * S.shape[1]
    assert np.array_equal(grid_ref.apply(X, S), S)
    v = np.arange(256, dtype=np.uint8)
    cube = np.stack(np.meshgrid(v[::5], v[::3], v, indexing="ij"), axis=-1).reshape(-1, 256, 3)      # every 8-bit value of R against a lattice of B and G
    px16 = all_values_16()
    for g in ((2, 2, 2), (3, 5, 4), (64, 64, 32)):
        Z = np.zeros(g + (3, 4))
        assert np.array_equal(grid_ref.apply(Z, cube), cube)
        assert np.array_equal(grid_ref.apply(Z, px16), px16)
        assert np.array_equal(grid_ref.apply(-Z, px16), px16)      # -0.0 entries as well


def test_node_rectangles_are_the_nearest_node_sets():
    """rule 3's closed form: the rows whose nearest node is n are exactly [lo(n), lo(n + 1))"""
    for H in (1, 2, 3, 7, 8, 9, 33, 56, 97, 257, 1000, 16384):
        for g in (2, 3, 5, 8, 33, 64):
            near = grid_ref.spatial_pos(H, g)[2]
            assert near.min() >= 0 and near.max() <= g - 1
            rows = 0
            for n in range(g):
                lo, hi = grid_ref.node_rect(n, g, H)
                assert 0 <= lo <= hi <= H and (near[lo:hi] == n).all()
                rows += hi - lo
            assert rows == H


def test_positions_interpolate_inside_the_grid():
    for n, g in ((1, 2), (7, 64), (16384, 64), (33, 5)):
        i, f, _ = grid_ref.spatial_pos(n, g)
        assert i.min() >= 0 and i.max() <= g - 2 and f.min() >= 0 and f.max() <= 2 * n
    for Z in (255, 65535):
        for gz in (2, 16, 32):
            Y = np.arange(Z + 1, dtype=np.int64)
            i, f, near = grid_ref.luma_pos(Y, gz, Z)
            assert i.min() >= 0 and i.max() <= gz - 2 and f.min() >= 0 and f.max() <= Z and near.min() == 0 and near.max() == gz - 1
    white = np.full((1, 1, 3), 65535, np.uint16)
    assert grid_ref.luma(white, 65535)[0, 0] == 65535 and grid_ref.luma(np.full((1, 1, 3), 255, np.uint8), 255)[0, 0] == 255


def test_splat_sums_do_not_depend_on_the_order_of_the_pixels(two):
    """the pixels of one spatial node's rectangle in any order give the same sums; any permutation of the whole picture keeps the totals over the spatial nodes"""
    S, O = two
    H, W = S.shape[:2]
    gy, gx, gz = 3, 5, 4
    ref = grid_ref.splat(S, O, gy, gx, gz)
    rng = np.random.default_rng(3)
    S2, O2 = S.copy(), O.copy()
    for ny in range(gy):
        y0, y1 = grid_ref.node_rect(ny, gy, H)
        for nx in range(gx):
            x0, x1 = grid_ref.node_rect(nx, gx, W)
            p = rng.permutation((y1 - y0) * (x1 - x0))
            S2[y0:y1, x0:x1] = S[y0:y1, x0:x1].reshape(-1, 3)[p].reshape(y1 - y0, x1 - x0, 3)
            O2[y0:y1, x0:x1] = O[y0:y1, x0:x1].reshape(-1, 3)[p].reshape(y1 - y0, x1 - x0, 3)
    assert not np.array_equal(S2, S) and np.array_equal(grid_ref.splat(S2, O2, gy, gx, gz), ref)
    p = rng.permutation(H * W)
    S3, O3 = S.reshape(-1, 3)[p].reshape(H, W, 3), O.reshape(-1, 3)[p].reshape(H, W, 3)
    tot = lambda s: s.reshape(gy * gx, gz, grid_ref.NSUM).sum(axis=0)
    assert np.array_equal(tot(grid_ref.splat(S3, O3, gy, gx, gz)), tot(ref))


def test_blur_keeps_mass_at_every_interpolation_corner(two):
    """after the blur each of the eight nodes a pixel interpolates from has a count"""
    S, O = two
    H, W = S.shape[:2]
    for g in ((8, 8, 8), (16, 16, 16), (64, 64, 32)):
        count = grid_ref.blur(grid_ref.splat(S, O, *g), *g)[:, grid_ref.COUNT].reshape(g)
        iy, ix, iz = grid_ref.spatial_pos(H, g[0])[0], grid_ref.spatial_pos(W, g[1])[0], grid_ref.luma_pos(grid_ref.luma(S, 255), g[2], 255)[0]
        for dy in (0, 1):
            for dx in (0, 1):
                for dz in (0, 1):
                    assert (count[(iy + dy)[:, None], (ix + dx)[None, :], iz + dz] > 0).all()
        assert grid_ref.blur(grid_ref.splat(S, O, *g), *g).max() < 1 << 48


def test_ldl_agrees_with_numpy_solve(two):
    """The reference's L D L^T against np.linalg.solve on the systems of the two-gradings fixture (FIXTURE_FITS: three grids, lambda at its two ends and at 16).
    Measured: the largest normwise backward error |M x - b| / (|M| |x| + |b|) of the reference is 1.42e-16 (LAPACK's on the same systems: 7.3e-17); asserted at 16
    times that. The two solutions then differ by at most cond(M) times the two backward errors (the perturbation bound), asserted with the same factor."""
    S, O = two
    worst = worst_np = 0.0
    for g, lam in FIXTURE_FITS:
        bl = grid_ref.blur(grid_ref.splat(S, O, *g), *g)
        bl = bl[bl[:, grid_ref.COUNT] > 0]
        M, B = grid_ref.system(bl, lam)
        X = grid_ref.ldl_solve(M, B)
        Xn = np.stack([np.linalg.solve(M, B[:, c, :, None])[..., 0] for c in range(3)], axis=1)
        nM = np.abs(M).sum(axis=2).max(axis=1)[:, None]
        nb = np.abs(B).max(axis=2)

        def backward(x):
            r = np.abs(np.einsum("nij,ncj->nci", M, x) - B).max(axis=2)
            den = nM * np.abs(x).max(axis=2) + nb
            return np.where(den > 0, r / np.where(den > 0, den, 1.0), 0.0)

        e, en = backward(X), backward(Xn)
        worst, worst_np = max(worst, float(e.max())), max(worst_np, float(en.max()))
        cond = np.linalg.cond(M, np.inf)[:, None]
        bound = cond * 2.0 * 16.0 * LDL_BACKWARD_ERROR * 2.0 * np.abs(Xn).max(axis=2)
        assert (np.abs(X - Xn).max(axis=2) <= bound + 1e-300).all(), (g, lam)
    print("largest backward error: L D L^T %.3g, numpy %.3g" % (worst, worst_np))
    assert worst <= 16.0 * LDL_BACKWARD_ERROR


def test_a_flat_patch_gets_a_pure_offset():
    """the ridge acts on the linear part only: one colour everywhere, shifted by a constant, gives the offset and (nearly) no linear part"""
    S = np.full((16, 16, 3), 100, np.uint8)
    O = np.full((16, 16, 3), 130, np.uint8)
    X, _, _ = grid_ref.fit(S, O, 2, 2, 2, 65536.0)
    assert mae(grid_ref.apply(X, S), O) == 0.0
    live = X[..., 3] != 0
    assert live.any() and np.abs(X[..., :3]).max() < 1e-3 and np.abs(X[..., 3][live] - 30.0).max() < 1.0


def test_two_gradings_fixture(two):
    """Measured (mean absolute error in grey levels): the untouched source 5.9, lut_ref.fit at N = 17, lambda = 0.1: 2.84; the 8 x 8 x 8 grid at lambda = 16: 0.73, the
    same grid on the 4 x pixel-replicated source 0.73; 16 x 16 x 16: 0.33."""
    S, O = two
    lut = lut_ref.fit(S.reshape(-1, 3), O.reshape(-1, 3), 17, 0.1)[0]
    e_lut = mae(lut_ref.apply(lut, 17, S.reshape(-1, 3)), O.reshape(-1, 3))
    X = grid_ref.fit(S, O, 8, 8, 8, 16.0)[0]
    e_grid = mae(grid_ref.apply(X, S), O)
    S4, O4 = (np.repeat(np.repeat(a, 4, axis=0), 4, axis=1) for a in (S, O))
    e_grid4 = mae(grid_ref.apply(X, S4), O4)
    e16 = mae(grid_ref.apply(grid_ref.fit(S, O, 16, 16, 16, 16.0)[0], S), O)
    print("source %.2f, table N = 17 %.2f, grid 8^3 %.2f, on the 4 x source %.2f, grid 16^3 %.2f" % (mae(S, O), e_lut, e_grid, e_grid4, e16))
    assert e_grid < 0.5 * e_lut
    assert e_grid4 < 0.5 * e_lut


def test_16_bit_apply_agrees_with_the_8_bit_apply(two):
    """a grid constant along z: both applies round the same real value, the bound of tests/test_gpu_lut16.py holds. Fitted grids (coefficients change along z, and the
    16-bit luma position is finer than the 8-bit one): the figure is printed, not asserted — measured 0.51 grey levels on the 8 x 8 x 8 fit of the fixture"""
    S, O = two
    rng = np.random.default_rng(8)
    u = rng.integers(0, 256, (64, 80, 3)).astype(np.uint8)
    u16 = u.astype(np.uint16) * 257
    for g in ((2, 2, 2), (8, 8, 8), (5, 7, 32)):
        X = np.repeat(rng.normal(0.0, 0.2, g[:2] + (1, 3, 4)), g[2], axis=2)
        X[..., 3] = X[..., 3] * 100.0
        worst = np.abs(grid_ref.apply(X, u16).astype(np.float64) / 257.0 - grid_ref.apply(X, u).astype(np.float64)).max()
        print("constant along z, grid %s: max |o16 / 257 - o8| = %.5f" % (g, worst))
        assert worst <= CONSISTENCY_BOUND
    X = grid_ref.fit(S, O, 8, 8, 8, 16.0)[0]
    worst = np.abs(grid_ref.apply(X, S.astype(np.uint16) * 257).astype(np.float64) / 257.0 - grid_ref.apply(X, S).astype(np.float64)).max()
    print("fitted 8 x 8 x 8 grid: max |o16 / 257 - o8| = %.5f" % worst)
