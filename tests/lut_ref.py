"""numpy reference of the 3D colour look-up tables (SPEC §6.6): the integer splat, the multigrid solve in the SPEC's exact order of operations, the trilinear apply
and a .cube reader / writer. Every floating-point operation is a single IEEE binary64 operation in the order the SPEC fixes (numpy never contracts), so the GPU
results are compared with these bit for bit. `direct` is the float64 sparse direct solve of the same normal equations, the yardstick of the solve's error."""
import numpy as np

SIZES = (3, 5, 9, 17, 33, 65)
W3 = 255 ** 3            # 16581375: the sum of a pixel's eight integer weights
SWEEPS = 2
CYCLES = 17              # V(2,2) cycles: SPEC §6.6 rule 7
MAX_PIXELS = 1 << 26


def _axis(v, N):
    t = v.astype(np.int64) * (N - 1)
    i = np.minimum(t // 255, N - 2)
    return i, t - 255 * i


def corners(bgr, N):
    """the eight (node index, integer weight) pairs of every pixel, corner order db outer, dg, dr inner; bgr [npix, 3] uint8"""
    bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
    (ib, fb), (ig, fg), (ir, fr) = _axis(bgr[:, 0], N), _axis(bgr[:, 1], N), _axis(bgr[:, 2], N)
    out = []
    for db in (0, 1):
        for dg in (0, 1):
            for dr in (0, 1):
                w = (fb if db else 255 - fb) * (fg if dg else 255 - fg) * (fr if dr else 255 - fr)
                out.append((((ib + db) * N + ig + dg) * N + ir + dr, w))
    return out


def splat(src, res, N):
    """W [N^3] uint64 and R [N^3, 3] int64 of source / result images [npix, 3] uint8 (BGR)"""
    assert N in SIZES
    src = np.ascontiguousarray(src, np.uint8).reshape(-1, 3)
    res = np.ascontiguousarray(res, np.uint8).reshape(-1, 3)
    assert src.shape == res.shape and 1 <= len(src) <= MAX_PIXELS
    diff = res.astype(np.int64) - src.astype(np.int64)
    W = np.zeros(N ** 3, np.int64)
    R = np.zeros((N ** 3, 3), np.int64)
    for idx, w in corners(src, N):
        np.add.at(W, idx, w)
        np.add.at(R, idx, w[:, None] * diff)
    return W.astype(np.uint64), R


def level_sizes(N):
    out = [N]
    while out[-1] > 3:
        out.append((out[-1] + 1) // 2)
    return out


def _degree(n):
    d = np.full(n, 2.0)
    d[0] = d[-1] = 1.0
    return d[:, None, None] + d[None, :, None] + d[None, None, :]


OFFS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]     # stencil entry e = (dz + 1) * 9 + (dy + 1) * 3 + dx + 1; 13 is the centre


def _shift(d):
    """(slice of the nodes whose neighbour at offset d is inside, slice of those neighbours)"""
    return {-1: (slice(1, None), slice(None, -1)), 0: (slice(None), slice(None)), 1: (slice(None, -1), slice(1, None))}[d]


def fine_operator(W, N, lam):
    """A_0 [N, N, N, 27]: omega + lam * deg in the centre, -lam on the six in-grid neighbours, 0.0 elsewhere"""
    A = np.zeros((N, N, N, 27))
    A[..., 13] = (W.astype(np.float64) / float(W3)).reshape(N, N, N) + float(lam) * _degree(N)
    for e, d in enumerate(OFFS):
        if abs(d[0]) + abs(d[1]) + abs(d[2]) == 1:
            (sz, _), (sy, _), (sx, _) = _shift(d[0]), _shift(d[1]), _shift(d[2])
            A[sz, sy, sx, e] = -float(lam)
    return A


def apply_op(A, x):
    """A x with the 27 taps summed in stencil order, those outside the grid skipped (x: [n, n, n, C])"""
    y = np.zeros_like(x)
    for e, d in enumerate(OFFS):
        (sz, tz), (sy, ty), (sx, tx) = _shift(d[0]), _shift(d[1]), _shift(d[2])
        y[sz, sy, sx] += A[sz, sy, sx, e, None] * x[tz, ty, tx]
    return y


def _residual(A, x, b):
    return b - apply_op(A, x)


def smoother_divisor(A):
    """q = max(1.25 A_ii, 0.625 sum_e |A_ie|): damped Jacobi (0.8) where the row is a Laplacian's, the l1 smoother where the consistent mass term dominates"""
    l1 = np.zeros(A.shape[:3])
    for e in range(27):
        l1 += np.abs(A[..., e])
    return np.maximum(1.25 * A[..., 13], 0.625 * l1)


def _jacobi(A, q, x, b):
    return x + _residual(A, x, b) / q[..., None]


_R_SL = {-1: (slice(1, None), slice(1, None, 2), 0.5), 0: (slice(None), slice(0, None, 2), 1.0), 1: (slice(None, -1), slice(1, None, 2), 0.5)}


def restrict(r):
    """full weighting without scaling (the transpose of `prolong`): taps db outer, dg, dr inner from -1 to 1, those outside the grid skipped"""
    n = r.shape[0]
    m = (n + 1) // 2
    acc = np.zeros((m, m, m) + r.shape[3:])
    for dz, dy, dx in OFFS:
        (cz, fz, wz), (cy, fy, wy), (cx, fx, wx) = _R_SL[dz], _R_SL[dy], _R_SL[dx]
        acc[cz, cy, cx] += (wz * wy * wx) * r[fz, fy, fx]
    return acc


_P_TAPS = {0: [(slice(None), 1.0)], 1: [(slice(None, -1), 0.5), (slice(1, None), 0.5)]}


def prolong(e):
    """trilinear interpolation to the finer lattice: per axis an even node copies its coarse node, an odd one takes half of each neighbour, taps b outer, r inner"""
    m = e.shape[0]
    n = 2 * m - 1
    out = np.zeros((n, n, n) + e.shape[3:])
    for pz in (0, 1):
        for py in (0, 1):
            for px in (0, 1):
                acc = np.zeros_like(out[pz::2, py::2, px::2])
                for sz, wz in _P_TAPS[pz]:
                    for sy, wy in _P_TAPS[py]:
                        for sx, wx in _P_TAPS[px]:
                            acc += (wz * wy * wx) * e[sz, sy, sx]
                out[pz::2, py::2, px::2] = acc
    return out


def galerkin(A):
    """P^T A P as a 27-point stencil on the coarser lattice: entry (I, delta) = sum over a (outer) and e (inner), both in stencil order, of
    P(a) P(b) A[2 I + a, e] with b = a + e - 2 delta inside {-1, 0, 1}^3, P(a) = 2^-(|a_b| + |a_g| + |a_r|); fine nodes outside the grid skipped"""
    n = A.shape[0]
    m = (n + 1) // 2
    Ac = np.zeros((m, m, m, 27))
    for k, dl in enumerate(OFFS):
        for a in OFFS:
            (cz, fz, wz), (cy, fy, wy), (cx, fx, wx) = _R_SL[a[0]], _R_SL[a[1]], _R_SL[a[2]]
            for e, d in enumerate(OFFS):
                b = (a[0] + d[0] - 2 * dl[0], a[1] + d[1] - 2 * dl[1], a[2] + d[2] - 2 * dl[2])
                if max(abs(b[0]), abs(b[1]), abs(b[2])) > 1:
                    continue
                w = wz * wy * wx * 0.5 ** (abs(b[0]) + abs(b[1]) + abs(b[2]))
                Ac[cz, cy, cx, k] += w * A[fz, fy, fx, e]
    return Ac


def _ldl(A):
    L = [[0.0] * 27 for _ in range(27)]
    d = [0.0] * 27
    for j in range(27):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * L[j][k]) * d[k]
        d[j] = dj
        for i in range(j + 1, 27):
            v = A[i][j]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = v / dj
    return L, d


def _ldl_solve(L, d, b):
    x = [0.0] * 27
    for i in range(27):
        v = b[i]
        for k in range(i):
            v = v - L[i][k] * x[k]
        x[i] = v
    for i in range(27):
        x[i] = x[i] / d[i]
    for i in range(26, -1, -1):
        v = x[i]
        for k in range(i + 1, 27):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x


def solve(W, R, N, lam, cycles=CYCLES, history=None):
    """D [N^3, 3] float64: `cycles` V(2,2) cycles of SPEC §6.6 rule 6 from D = 0. history (a list) receives D after every cycle"""
    sizes = level_sizes(N)
    A = [fine_operator(W, N, lam)]
    for _ in sizes[1:]:
        A.append(galerkin(A[-1]))
    # the coarsest lattice has 27 nodes: its stencil is the dense matrix, row i, column i + offset, 0.0 between nodes two apart on an axis
    dense = [[0.0] * 27 for _ in range(27)]
    for z in range(3):
        for y in range(3):
            for x in range(3):
                for e, d in enumerate(OFFS):
                    zz, yy, xx = z + d[0], y + d[1], x + d[2]
                    if 0 <= zz < 3 and 0 <= yy < 3 and 0 <= xx < 3:
                        dense[(z * 3 + y) * 3 + x][(zz * 3 + yy) * 3 + xx] = float(A[-1][z, y, x, e])
    L, d = _ldl(dense)
    q = [smoother_divisor(a) for a in A]
    b0 = (R.astype(np.float64) / float(W3)).reshape(N, N, N, 3)

    def coarse(b):
        x = np.zeros_like(b)
        for c in range(3):
            x[..., c] = np.array(_ldl_solve(L, d, [float(v) for v in b[..., c].reshape(-1)])).reshape(3, 3, 3)
        return x

    def vcycle(k, x, b):
        if k == len(sizes) - 1:
            return coarse(b)
        for _ in range(SWEEPS):
            x = _jacobi(A[k], q[k], x, b)
        bc = restrict(_residual(A[k], x, b))
        x = x + prolong(vcycle(k + 1, np.zeros_like(bc), bc))
        for _ in range(SWEEPS):
            x = _jacobi(A[k], q[k], x, b)
        return x

    x = np.zeros_like(b0)
    for _ in range(cycles):
        x = vcycle(0, x, b0)
        if history is not None:
            history.append(x.reshape(-1, 3).copy())
    return x.reshape(-1, 3)


def direct(W, R, N, lam):
    """the float64 sparse direct solve of the normal equations (scipy), the yardstick of `solve`"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n = N ** 3
    idx = np.arange(n).reshape(N, N, N)
    rows, cols = [], []
    for a, b in ((idx[1:], idx[:-1]), (idx[:, 1:], idx[:, :-1]), (idx[:, :, 1:], idx[:, :, :-1])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.coo_matrix((np.full(len(rows), -float(lam)), (rows, cols)), shape=(n, n)).tocsc()
    A = A + sp.diags(W.astype(np.float64) / W3 + lam * _degree(N).ravel())
    if not R.any():                                      # a zero right-hand side of an SPD system: the solution is zero, no factorisation needed
        return np.zeros((n, 3))
    # the minimum-degree ordering of A + A^T: a fifth of the default ordering's fill on this symmetric 7-point matrix
    lu = spl.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    return lu.solve(R.astype(np.float64) / W3)


def node_colors(N):
    """[N^3, 3] float64: the node colours 255 i / (N - 1) in BGR order, index [ib][ig][ir]"""
    g = np.arange(N, dtype=np.float64) * 255.0 / (N - 1)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([b, gg, r], axis=-1).reshape(-1, 3)


def table(D, N):
    return (node_colors(N) + D).astype(np.float32)


def fit(src, res, N, lam, cycles=CYCLES):
    W, R = splat(src, res, N)
    D = solve(W, R, N, lam, cycles)
    return table(D, N), W, R, D


def identity(N):
    return node_colors(N).astype(np.float32)


def apply(lut, N, bgr):
    """out [npix, 3] uint8: the double sum over the eight corners (db outer, dr inner) of w * LUT, / 255^3, clamped to [0, 255] and rounded to nearest even"""
    lut = np.ascontiguousarray(lut, np.float32).reshape(N ** 3, 3).astype(np.float64)
    acc = None
    for idx, w in corners(bgr, N):
        term = w.astype(np.float64)[:, None] * lut[idx]
        acc = term if acc is None else acc + term
    v = acc / float(W3)
    v = np.where(v > 0.0, v, 0.0)
    v = np.where(v < 255.0, v, 255.0)
    return np.rint(v).astype(np.uint8)


def write_cube(path, lut, N):
    """LUT_3D_SIZE N, then N^3 lines "R G B" in [0, 1], red fastest: the table's own order with the channels turned round"""
    lut = np.ascontiguousarray(lut, np.float32).reshape(N ** 3, 3)
    with open(path, "w") as f:
        f.write("LUT_3D_SIZE %d\n" % N)
        for b, g, r in lut:
            f.write("%s %s %s\n" % tuple("%.9g" % np.float32(min(max(np.float32(v) / np.float32(255.0), np.float32(0.0)), np.float32(1.0))) for v in (r, g, b)))


def read_cube(path):
    """(N, values [N^3, 3] float32 in BGR order, as written: value / 255 clamped to [0, 1])"""
    N, rows = None, []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            if line.startswith("LUT_3D_SIZE"):
                N = int(line.split()[1])
            elif line[0].isdigit() or line[0] in "-.":
                rows.append([np.float32(t) for t in line.split()])
    a = np.array(rows, np.float32)
    assert N is not None and a.shape == (N ** 3, 3)
    return N, np.ascontiguousarray(a[:, ::-1])


def cube_values(lut):
    """what write_cube prints for a table: fp32 value / 255 (fp32 division) clamped to [0, 1], BGR order"""
    v = np.ascontiguousarray(lut, np.float32) / np.float32(255.0)
    return np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0)).astype(np.float32)
