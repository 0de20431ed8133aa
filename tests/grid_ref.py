"""numpy reference of the local colour grids (SPEC §6.22): a bilateral grid of 3 x 4 affine BGR maps over (row, column, luma), fitted from a (source, result) pair by
an integer splat, an integer blur and one 4 x 4 L D L^T solve per node, and applied to 8-bit or 16-bit pixels of any size. Integer operations are exact; every
floating-point operation is a single IEEE binary64 operation in the order the SPEC fixes (numpy never contracts), elementwise over nodes, so the GPU results are
compared with these bit for bit."""
import numpy as np

NSUM = 22                # 10 Gram sums, then 12 right-hand sides [c][j]
MAX_PIXELS = 1 << 26
MAX_SIDE = 16384
GRAM = [(j, k) for j in range(4) for k in range(j, 4)]        # the 10 distinct sums s_j s_k in their order; (3, 3) is the count, index 9
COUNT = 9


def grid_ok(gy, gx, gz):
    return 2 <= gy <= 64 and 2 <= gx <= 64 and 2 <= gz <= 32


def spatial_pos(n, g):
    """rule 2 for the indices 0 .. n - 1 of a side of n pixels under g nodes: (cell i, f in [0, 2n), nearest node), int64"""
    t = (2 * np.arange(n, dtype=np.int64) + 1) * (g - 1)
    i = np.minimum(t // (2 * n), g - 2)
    return i, t - 2 * n * i, (t + n) // (2 * n)


def luma(px, Z):
    """Y = (29 B + 150 G + 77 R + 128) >> 8 on the raw values, px [..., 3] -> int64 in [0, Z]"""
    p = px.astype(np.int64)
    return (29 * p[..., 0] + 150 * p[..., 1] + 77 * p[..., 2] + 128) >> 8


def luma_pos(Y, gz, Z):
    """(cell i, f in [0, Z], nearest node) of a luma"""
    t = Y * (gz - 1)
    i = np.minimum(t // Z, gz - 2)
    return i, t - Z * i, (2 * t + Z) // (2 * Z)


def node_rect(n, g, H):
    """the rows [lo, hi) whose nearest node is n, in closed form: lo(n) = ceil((2 H n - H) / (g - 1)) / 2, lo(0) = 0, lo(g) = H"""
    def lo(k):
        if k <= 0:
            return 0
        if k >= g:
            return H
        a = 2 * H * k - H
        return min(H, ((a + g - 2) // (g - 1)) // 2)
    return lo(n), lo(n + 1)


def splat(S, O, gy, gx, gz):
    """sums [gy * gx * gz, 22] int64 of 8-bit images S, O [H, W, 3]: weight 1 at every pixel's nearest node"""
    S = np.ascontiguousarray(S, np.uint8)
    O = np.ascontiguousarray(O, np.uint8)
    assert S.ndim == 3 and S.shape == O.shape and S.shape[2] == 3 and grid_ok(gy, gx, gz)
    H, W = S.shape[:2]
    assert 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and H * W <= MAX_PIXELS
    ny, nx = spatial_pos(H, gy)[2], spatial_pos(W, gx)[2]
    nz = luma_pos(luma(S, 255), gz, 255)[2]
    node = ((ny[:, None] * gx + nx[None, :]) * gz + nz).reshape(-1)
    s = np.concatenate([S.astype(np.int64), np.ones((H, W, 1), np.int64)], axis=2).reshape(-1, 4)
    d = (O.astype(np.int64) - S.astype(np.int64)).reshape(-1, 3)
    terms = [s[:, j] * s[:, k] for j, k in GRAM] + [s[:, j] * d[:, c] for c in range(3) for j in range(4)]
    sums = np.zeros((gy * gx * gz, NSUM), np.int64)
    np.add.at(sums, node, np.stack(terms, axis=1))
    return sums


def blur(sums, gy, gx, gz):
    """one integer [1 2 1] pass along each of the three axes, out-of-grid taps dropped"""
    a = sums.reshape(gy, gx, gz, NSUM).astype(np.int64)
    for ax in range(3):
        b = 2 * a
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[ax], hi[ax] = slice(None, -1), slice(1, None)
        b[tuple(hi)] += a[tuple(lo)]
        b[tuple(lo)] += a[tuple(hi)]
        a = b
    return a.reshape(-1, NSUM)


def ldl_solve(M, B):
    """x of M x = b for M [n, 4, 4] (the lower triangle is read), B [n, 3, 4] -> [n, 3, 4]: L D L^T without pivoting in SPEC §6.6 rule 6's order of operations"""
    n = M.shape[0]
    L = np.zeros((n, 4, 4))
    d = np.zeros((n, 4))
    for j in range(4):
        dj = M[:, j, j].copy()
        for k in range(j):
            dj = dj - (L[:, j, k] * L[:, j, k]) * d[:, k]
        d[:, j] = dj
        for i in range(j + 1, 4):
            v = M[:, i, j].copy()
            for k in range(j):
                v = v - (L[:, i, k] * L[:, j, k]) * d[:, k]
            L[:, i, j] = v / dj
    X = np.zeros((n, 3, 4))
    for c in range(3):
        x = np.zeros((n, 4))
        for i in range(4):
            v = B[:, c, i].copy()
            for k in range(i):
                v = v - L[:, i, k] * x[:, k]
            x[:, i] = v
        for i in range(4):
            x[:, i] = x[:, i] / d[:, i]
        for i in range(3, -1, -1):
            v = x[:, i].copy()
            for k in range(i + 1, 4):
                v = v - L[:, k, i] * x[:, k]
            x[:, i] = v
        X[:, c] = x
    return X


def system(blurred, lam):
    """(M [n, 4, 4], B [n, 3, 4]) of the nodes of `blurred`: the Gram matrix as doubles with lam * (double)count added on the linear part's diagonal"""
    n = blurred.shape[0]
    M = np.zeros((n, 4, 4))
    for idx, (j, k) in enumerate(GRAM):
        M[:, j, k] = M[:, k, j] = blurred[:, idx].astype(np.float64)
    r = float(lam) * blurred[:, COUNT].astype(np.float64)
    for j in range(3):
        M[:, j, j] = M[:, j, j] + r
    return M, blurred[:, 10:].astype(np.float64).reshape(n, 3, 4)


def solve(blurred, lam):
    """X [nodes, 3, 4] float64; a node whose blurred count is 0 gets X = 0"""
    live = blurred[:, COUNT] > 0
    X = np.zeros((blurred.shape[0], 3, 4))
    if live.any():
        M, B = system(blurred[live], lam)
        X[live] = ldl_solve(M, B)
    return X


def fit(S, O, gy, gx, gz, lam):
    """(X [gy, gx, gz, 3, 4], sums, blurred)"""
    sums = splat(S, O, gy, gx, gz)
    bl = blur(sums, gy, gx, gz)
    return solve(bl, lam).reshape(gy, gx, gz, 3, 4), sums, bl


def apply(X, img):
    """the grid X [gy, gx, gz, 3, 4] on an image [H, W, 3] uint8 or uint16 -> the image of the same shape and dtype (rule 6)"""
    X = np.ascontiguousarray(X, np.float64)
    gy, gx, gz = X.shape[:3]
    assert X.shape[3:] == (3, 4) and img.ndim == 3 and img.shape[2] == 3 and img.dtype in (np.uint8, np.uint16)
    Z, K = (255, 1.0) if img.dtype == np.uint8 else (65535, 257.0)
    H, W = img.shape[:2]
    iy, fy, _ = spatial_pos(H, gy)
    ix, fx, _ = spatial_pos(W, gx)
    iz, fz, _ = luma_pos(luma(img, Z), gz, Z)
    Xf = X.reshape(-1, 12)
    acc = np.zeros((H, W, 12))
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in (0, 1):
            wy = (fy if dy else 2 * H - fy)[:, None]
            for dx in (0, 1):
                wx = (fx if dx else 2 * W - fx)[None, :]
                for dz in (0, 1):
                    w = (wy * wx) * (fz if dz else Z - fz)
                    node = (((iy + dy)[:, None] * gx + (ix + dx)[None, :]) * gz + iz + dz)
                    acc = acc + w.astype(np.float64)[..., None] * Xf[node]
        s = img.astype(np.float64)
        Dn = float(2 * H) * float(2 * W) * float(Z)
        out = np.empty((H, W, 3))
        for c in range(3):
            a = acc[..., 4 * c:4 * c + 4]
            t = ((a[..., 0] * s[..., 0] + a[..., 1] * s[..., 1]) + a[..., 2] * s[..., 2]) + a[..., 3] * K
            out[..., c] = s[..., c] + t / Dn
        out = np.where(out > 0.0, out, 0.0)               # A1's cast: a NaN becomes 0
        out = np.where(out < float(Z), out, float(Z))
    return np.rint(out).astype(img.dtype)


def two_gradings(h=56, w=64, seed=5):
    """the fixture of SPEC §6.22: a smooth noisy source and a result whose left and right halves get opposite gradings, blended over 3 px at the middle column"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 80 * np.sin(xx / 9.0 + 0.3) * np.cos(yy / 11.0), 120 + 90 * np.sin(yy / 7.0 + xx / 23.0), 135 + 70 * np.cos(xx / 13.0 - yy / 17.0)], axis=-1)
    Sf = base + rng.normal(0.0, 12.0, base.shape)
    S = np.clip(np.rint(Sf), 0, 255).astype(np.uint8)
    s = S.astype(np.float64)
    A = s * np.array([1.15, 0.9, 0.8]) + np.array([-20.0, 10.0, 30.0])
    B = s * np.array([0.8, 1.1, 1.2]) + np.array([25.0, -15.0, -25.0])
    t = 1.0 / (1.0 + np.exp(-(xx - (w - 1) / 2.0) / 3.0))
    O = np.clip(np.rint(A * (1 - t[..., None]) + B * t[..., None]), 0, 255).astype(np.uint8)
    return S, O
