"""Region models (SPEC §6.17): the rules restated in numpy. A model is (tap, rows_in, rows_out): the kept seed rows of region_select_ref's rule 3. The quantised rows and
the score are region_select_ref's, the resize region_ref.resize_u8c1, the snap region_snap_ref.snap: those modules are imported, not edited. The only arithmetic of its
own is R2 and R3. Shared by tests/test_region_model.py (CPU) and tests/test_gpu_region_model.py."""
import numpy as np

import region_ref
import region_select_ref as sel
import region_snap_ref as rs

SHARPNESS, FLOOR_PERMILLE, MARGIN, SNAP_ITERS = 1024, 700, 32, 1        # nct_region_refind_params_default
SNAP = (rs.RADIUS, rs.SIGMA, rs.BINARY)
MAX_ROWS = 65536


def fit(orc, src, strokes, ws, bs, tap=sel.TAP, max_seeds=sel.MAX_SEEDS, feat=None):
    """nct_region_model_fit -> (tap, rows_in, rows_out): §6.16 rules 1 to 3, the kept rows in raster order"""
    S, T = np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(strokes, np.uint8)
    F = feat if feat is not None else orc.vgg19_features(S, ws, bs, deepest_tap=tap)[tap - 1]
    q = sel.quantize(orc, F)
    _, i_in, i_out = sel.seed_cells(T, tap, max_seeds)
    if len(i_in) == 0:
        raise sel.NoInsideSeed()
    return tap, q[i_in].copy(), q[i_out].copy()


def add(model, other):
    """nct_region_model_add: the other image's kept rows behind the model's"""
    assert model[0] == other[0]
    rows_in, rows_out = np.concatenate([model[1], other[1]]), np.concatenate([model[2], other[2]])
    assert len(rows_in) <= MAX_ROWS and len(rows_out) <= MAX_ROWS
    return model[0], rows_in, rows_out


def refind(orc, score, shape, prior=None, margin=MARGIN):
    """R1 to R3: score [ht][wt] bytes, shape (H, W) not smaller than the grid, prior [H][W] bytes or None -> [H][W] bytes"""
    m = np.ascontiguousarray(score, np.uint8)
    H, W = shape
    assert H >= m.shape[0] and W >= m.shape[1] and 0 <= margin <= 128
    r = region_ref.resize_u8c1(orc, m, H, W)
    if prior is None:
        return r
    ri = r.astype(np.int64)
    confident = (ri >= 128 + margin) | (ri < 128 - margin)
    return np.where(confident, r, np.asarray(prior, np.uint8)).astype(np.uint8)


def apply(orc, model, src, ws, bs, prior=None, sharpness=SHARPNESS, floor_permille=FLOOR_PERMILLE, margin=MARGIN, snap_iters=SNAP_ITERS, snap=SNAP, feat=None, guide=None):
    """nct_region_model_apply -> (the matte, {"q", "score", "refound"}). feat: the model's tap of the oracle's VGG19 of src where the caller already holds it.
    guide (a full-resolution sequence, rule S4): the frame at the size frames arrive, src being its working-size form — the re-find goes from src's tap grid straight
    to the guide's size, where the prior lives and the snap passes run"""
    tap, rows_in, rows_out = model
    S = np.ascontiguousarray(src, np.uint8)
    G = S if guide is None else np.ascontiguousarray(guide, np.uint8)
    h, w = S.shape[:2]
    ht, wt = sel.grid(h, w, tap)
    F = feat if feat is not None else orc.vgg19_features(S, ws, bs, deepest_tap=tap)[tap - 1]
    assert F.shape == (sel.TAP_C[tap - 1], ht, wt)
    q = sel.quantize(orc, F)
    m = sel.score(q, rows_in, rows_out, sharpness, floor_permille).reshape(ht, wt)
    R = refind(orc, m, G.shape[:2], prior, margin)
    M = R
    lab = orc.bgr2lab(G) if snap_iters else None
    for _ in range(snap_iters):
        M = rs.snap(M, lab, *snap)
    return M, {"q": q, "score": m, "refound": R}


def sequence_mattes(orc, model, ws, bs, frames, kinds, fields, seq_snap, zero_at=(), guides=None, given=None, **apply_kw):
    """rules S1 to S6 over a clip with tracking on -> the matte in force after every frame (None while there is none). frames: at the working size; guides: the frames at
    the size frames arrive (None: the same); kinds[t]: "P" a propagated frame, else a full one; fields[t]: the field of the top level run of frame t (None: motion
    off); seq_snap: nct_seq_set_region_snap's (r, sigma, binary) or None; zero_at: the frames without state beside frame 0 (after a reset, CUT frames); given[t]: the
    matte nct_seq_set_region gives before frame t. The chain: carry -> snap -> re-find on full frames, the carry and the snap alone on propagated ones"""
    import seq_track_ref as tr
    guides = frames if guides is None else guides
    out, cur = [], None
    for t, f in enumerate(frames):
        state = t > 0 and t not in zero_at
        fresh = given is not None and given[t] is not None
        if fresh:
            cur = np.ascontiguousarray(given[t], np.uint8)
        if cur is not None and not fresh and state:
            if fields[t] is not None:
                cur = tr.matte_warp(cur, fields[t])
            if seq_snap is not None:
                cur = rs.snap(cur, orc.bgr2lab(np.ascontiguousarray(guides[t], np.uint8)), *seq_snap)
        if kinds[t] != "P" and not fresh:
            cur = apply(orc, model, f, ws, bs, prior=cur if state else None, guide=guides[t], **apply_kw)[0]
        out.append(cur)
    return out


def moved(dy, dx, seed, hi=170, lo=90, period=3, occluder=None):
    """region_select_ref.texture_fixture's formula with the ellipse and its stripes shifted by (dy, dx) under fresh noise -> (image, the true object). occluder: a
    column range (x0, x1) overwritten with the checkerboard; the truth is then the ellipse minus that bar"""
    H, W = 96, 112
    yy, xx = np.mgrid[0:H, 0:W]
    obj = ((yy - 50 - dy) / 30) ** 2 + ((xx - 60 - dx) / 36) ** 2 < 1
    inside = np.where(((xx - dx + yy - dy) // period) % 2 == 0, hi, lo)
    outside = np.where(((xx // 4) + (yy // 4)) % 2 == 0, 170, 90)
    if occluder is not None:
        bar = (xx >= occluder[0]) & (xx < occluder[1])
        obj = obj & ~bar
    g = np.where(obj, inside, outside)
    img = np.clip(np.repeat(g[:, :, None], 3, axis=2) + np.random.default_rng(seed).integers(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img), obj


# ---- the seam cases of the GPU test: (grid, target) pairs, score kinds, margins
REFIND_CASES = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((3, 4), (3, 4)), ((28, 32), (56, 64)), ((29, 34), (57, 67)), ((4, 5), (57, 67)), ((7, 9), (40, 300)), ((33, 40), (34, 41))]
MARGINS = (0, 1, 32, 127, 128)
SCORE_KINDS = ("random", "edges")


def refind_inputs(case, kind, margin, seed=31):
    """-> (score [ht][wt], prior [H][W]). random: random bytes; edges: bytes drawn from {127 - g, 128 - g, 127 + g, 128 + g}, g the margin: both sides of both
    comparisons of R2 (clipped to a byte at g = 128)"""
    (ht, wt), (H, W) = case
    rng = np.random.default_rng(seed + 7 * ht + 13 * W + margin + (0 if kind == "random" else 1000))
    if kind == "random":
        score = rng.integers(0, 256, (ht, wt)).astype(np.uint8)
    else:
        vals = np.clip(np.array([127 - margin, 128 - margin, 127 + margin, 128 + margin]), 0, 255).astype(np.uint8)
        score = vals[rng.integers(0, 4, (ht, wt))]
    prior = rng.integers(0, 256, (H, W)).astype(np.uint8)
    return score, prior
