"""Region selection from strokes (SPEC §6.16): the rule restated in numpy. F comes from the oracle's VGG19, N1 from orc_feat_normalize, the resize from
region_ref.resize_u8c1 and the snap from region_snap_ref.snap; the dot products are int64 matrix products. No new reference arithmetic beside the rule: those modules
are imported, not edited. Shared by tests/test_region_select.py (CPU) and tests/test_gpu_region_select.py."""
import numpy as np

import region_ref
import region_snap_ref as rs

IN, OUT = 255, 128                                  # NCT_STROKE_IN, NCT_STROKE_OUT
TAP, SHARPNESS, FLOOR_PERMILLE, MAX_SEEDS, SNAP_ITERS = 2, 1024, 700, 4096, 1      # nct_region_select_params_default
SNAP = (rs.RADIUS, rs.SIGMA, rs.BINARY)
TAP_C = (64, 128, 256, 512, 512)
NONE, IN_KEPT, OUT_KEPT, IN_DROPPED, OUT_DROPPED, MIXED = 0, 1, 2, 3, 4, 5          # nct_region_select_stages.cell


def grid(h, w, tap):
    return ((h - 1) >> (tap - 1)) + 1, ((w - 1) >> (tap - 1)) + 1


def quantize(orc, feat_chw):
    """rule 2: CHW fp32 -> [H*W][C] int16, rint(N1(F) * 32767) with the product in fp32; a non-finite u gives 0"""
    f = np.ascontiguousarray(feat_chw, np.float32)
    C = f.shape[0]
    with np.errstate(all="ignore"):
        u = orc.feat_normalize(f)
        t = u * np.float32(32767)
        assert t.dtype == np.float32
        q = np.where(np.isfinite(u), np.rint(t), np.float32(0)).astype(np.int16)
    return np.ascontiguousarray(q.reshape(C, -1).T)


def kept(n, max_seeds):
    """rule 3's subsample: which of the n seeds of a class, by raster rank, are kept"""
    i = np.arange(n, dtype=np.int64)
    if n <= max_seeds:
        return np.ones(n, bool)
    return (i + 1) * max_seeds // n > i * max_seeds // n


def seed_cells(strokes, tap, max_seeds=MAX_SEEDS):
    """rule 3 -> (cell codes [h_t][w_t], the kept inside seeds' cell indices in raster order, the kept outside seeds')"""
    T = np.asarray(strokes, np.uint8)
    h, w = T.shape
    ht, wt = grid(h, w, tap)
    has = []
    for v in (IN, OUT):
        ys, xs = np.nonzero(T == v)
        a = np.zeros(ht * wt, bool)
        a[(ys >> (tap - 1)) * wt + (xs >> (tap - 1))] = True
        has.append(a)
    code = np.zeros(ht * wt, np.uint8)
    code[has[0] & has[1]] = MIXED
    idx = []
    for a, b, yes, no in ((has[0], has[1], IN_KEPT, IN_DROPPED), (has[1], has[0], OUT_KEPT, OUT_DROPPED)):
        cells = np.nonzero(a & ~b)[0]
        k = kept(len(cells), max_seeds)
        code[cells[k]] = yes; code[cells[~k]] = no
        idx.append(cells[k])
    return code.reshape(ht, wt), idx[0], idx[1]


def score(q, seeds_in, seeds_out, sharpness=SHARPNESS, floor_permille=FLOOR_PERMILLE):
    """rule 4 without the seed-cell overwrite: int16 rows -> [cells] bytes"""
    Q = np.asarray(q, np.int16).astype(np.int64)
    s_in = (Q @ np.asarray(seeds_in, np.int16).astype(np.int64).T).max(axis=1)
    if seeds_out is not None and len(seeds_out):
        s_out = (Q @ np.asarray(seeds_out, np.int16).astype(np.int64).T).max(axis=1)
    else:
        s_out = np.full(len(Q), floor_permille * 2 ** 30 // 1000, np.int64)
    d = s_in - s_out
    return np.clip(128 + (d * sharpness + 2 ** 29) // 2 ** 30, 0, 255).astype(np.uint8)


def stamp(M, strokes):
    M = M.copy()
    M[strokes == IN] = 255
    M[strokes == OUT] = 0
    return M


class NoInsideSeed(Exception):
    pass


def select(orc, src, strokes, ws, bs, tap=TAP, sharpness=SHARPNESS, floor_permille=FLOOR_PERMILLE, max_seeds=MAX_SEEDS, snap_iters=SNAP_ITERS, snap=SNAP, feat=None):
    """nct_region_select -> (the matte, {"q", "cell", "score", "up"}). feat: tap `tap` of the oracle's VGG19 of src where the caller already holds it"""
    S, T = np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(strokes, np.uint8)
    h, w = T.shape
    ht, wt = grid(h, w, tap)
    F = feat if feat is not None else orc.vgg19_features(S, ws, bs, deepest_tap=tap)[tap - 1]
    assert F.shape == (TAP_C[tap - 1], ht, wt)
    q = quantize(orc, F)
    code, i_in, i_out = seed_cells(T, tap, max_seeds)
    if len(i_in) == 0:
        raise NoInsideSeed()
    m = score(q, q[i_in], q[i_out], sharpness, floor_permille).reshape(ht, wt)
    m[(code == IN_KEPT) | (code == IN_DROPPED)] = 255
    m[(code == OUT_KEPT) | (code == OUT_DROPPED)] = 0
    up = region_ref.resize_u8c1(orc, m, h, w)
    M = stamp(up, T)
    lab = orc.bgr2lab(S) if snap_iters else None
    for _ in range(snap_iters):
        M = stamp(rs.snap(M, lab, *snap), T)
    return M, {"q": q, "cell": code, "score": m, "up": up}


def colour_only(orc, src, strokes):
    """the rule this one replaces: per pixel the nearest stroke pixel in 8-bit Lab decides, inside where an IN pixel is strictly nearer than every OUT pixel"""
    lab = orc.bgr2lab(np.ascontiguousarray(src, np.uint8)).astype(np.int64)
    P = lab.reshape(-1, 3)
    d = [((P[:, None, :] - lab[strokes == v][None, :, :]) ** 2).sum(axis=-1).min(axis=1) for v in (IN, OUT)]
    return np.where(d[0] < d[1], 255, 0).astype(np.uint8).reshape(strokes.shape)


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return (a & b).sum() / (a | b).sum()


def texture_fixture():
    """two textures of the same two grey values and the same mean: diagonal stripes inside an ellipse, a checkerboard outside -> (image, strokes, the true object)"""
    H, W = 96, 112
    yy, xx = np.mgrid[0:H, 0:W]
    obj = ((yy - 50) / 30) ** 2 + ((xx - 60) / 36) ** 2 < 1
    inside = np.where(((xx + yy) // 3) % 2 == 0, 170, 90)
    outside = np.where(((xx // 4) + (yy // 4)) % 2 == 0, 170, 90)
    g = np.where(obj, inside, outside)
    img = np.clip(np.repeat(g[:, :, None], 3, axis=2) + np.random.default_rng(5).integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    T = np.zeros((H, W), np.uint8)
    T[48:53, 40:80] = IN
    T[4:8, 10:100] = OUT
    T[30:70, 4:8] = OUT
    return np.ascontiguousarray(img), T, obj


# the whole-call cases of the GPU test: the object clip's rectangle (region_snap_ref.OBJ_*) on a synth image of either size, and strokes with seeds of both classes
# beyond max_seeds = 7 at taps 1 to 3, a cell that holds both kinds from tap 2 on, another from tap 3 on (at tap 5 the two are one cell)
SIZES = ((56, 64), (57, 67))


def call_source(h, w):
    import synth
    img = synth.image(1000, h, w).copy()
    img[rs.OBJ_ROWS[0]:rs.OBJ_ROWS[1], rs.OBJ_COLS[0]:rs.OBJ_COLS[1]] = rs.OBJ_BGR
    return np.ascontiguousarray(img)


def call_strokes(h, w, outside=True):
    T = np.zeros((h, w), np.uint8)
    T[24:30, 14:34] = IN
    T[31, 37] = IN
    if outside:
        T[2:6, 4:60] = OUT
        T[44:54, 44:60] = OUT
        T[30, 36] = OUT            # with the IN pixel at (31, 37): one cell from tap 2 on
        T[25, 35] = OUT            # with the IN stroke's right end: one cell from tap 3 on
    return T
