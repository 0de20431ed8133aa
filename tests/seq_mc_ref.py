"""Motion-compensated frame sequences (SPEC §6.4): the search (rules 1-3) and the blend through a field (rule 4) restated in numpy, the composition of seq_ref with the
field carried from level to level, and the flicker metrics taken along a known pan. Shared by tests/test_seq_mc.py (CPU) and tests/test_gpu_seq_mc.py. Everything in the
search is integer arithmetic; the blend's doubles are seq_ref.blend's expressions, operation for operation."""
import numpy as np

import fullres_ref
import multi_ref
import seq_ref

RADIUS0, RADIUS, PENALTY = 3, 1, 1          # nct_seq_motion_default
P = 2                                       # patch half-width: 5 x 5 taps


def candidates(R):
    """(dy, dx) with |dy|, |dx| <= R in the order of rule 3: ascending (|dy| + |dx|, dy, dx)"""
    return sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda m: (abs(m[0]) + abs(m[1]), m[0], m[1]))


def centre(h, w, parent):
    """rule 1 -> (cy, cx) int64 [h][w]"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    if parent is None:
        return np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    par = np.asarray(parent, np.int16).astype(np.int64)
    ph, pw = par.shape[:2]
    m = par[np.minimum(yy >> 1, ph - 1), np.minimum(xx >> 1, pw - 1)]
    return np.clip(yy + 2 * m[..., 0], 0, h - 1) - yy, np.clip(xx + 2 * m[..., 1], 0, w - 1) - xx


def cost(L, Lp, my, mx):
    """rule 2 for a displacement per pixel -> (cost, n) int64 [h][w]"""
    L = np.asarray(L, np.uint8).astype(np.int64); Lp = np.asarray(Lp, np.uint8).astype(np.int64)
    h, w = L.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    c = np.zeros((h, w), np.int64); n = np.zeros((h, w), np.int64)
    for ty in range(-P, P + 1):
        for tx in range(-P, P + 1):
            qy, qx = yy + ty, xx + tx
            ry, rx = qy + my, qx + mx
            ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w) & (ry >= 0) & (ry < h) & (rx >= 0) & (rx < w)
            a = L[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
            b = Lp[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)]
            c += np.where(ok, np.abs(a - b).sum(axis=2), 0)
            n += ok
    return c, n


def motion(L, Lp, parent, R, penalty):
    """rules 1-3: L, Lp h x w x 3 uint8 (frame t, frame t-1), parent None or int16 [ph][pw][2] -> int16 [h][w][2] of (my, mx)"""
    h, w = np.asarray(L).shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    cy, cx = centre(h, w, parent)
    bK = bn = None
    by, bx = cy.copy(), cx.copy()
    for (dy, dx) in candidates(R):
        my, mx = cy + dy, cx + dx
        adm = (yy + my >= 0) & (yy + my < h) & (xx + mx >= 0) & (xx + mx < w)
        c, n = cost(L, Lp, my, mx)
        K = c + penalty * n * (abs(dy) + abs(dx))
        if bK is None:                                         # (0, 0): always admissible
            assert adm.all() and (n >= 1).all()
            bK, bn = K, n
            continue
        take = adm & (K * bn < bK * n)
        bK = np.where(take, K, bK); bn = np.where(take, n, bn)
        by = np.where(take, my, by); bx = np.where(take, mx, bx)
    return np.stack([by, bx], axis=2).astype(np.int16)


def blend_mc(x, x_prev, lab, lab_prev, tau, sigma, field):
    """rule 4: seq_ref.blend with L_(t-1) and X'_(t-1) read at p + m(p); a vector that leaves the grid is clamped to it. field None: seq_ref.blend.
    -> (X' [2][h*w][3], tau_p [h][w])"""
    if field is None:
        return seq_ref.blend(x, x_prev, lab, lab_prev, tau, sigma)
    lab = np.asarray(lab, np.uint8)
    h, w = lab.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    f = np.asarray(field, np.int16).astype(np.int64).reshape(h, w, 2)
    my = np.clip(yy + f[..., 0], 0, h - 1) - yy
    mx = np.clip(xx + f[..., 1], 0, w - 1) - xx
    cur = lab.astype(np.int64); old = np.asarray(lab_prev, np.uint8).astype(np.int64)
    D = np.zeros((h, w), np.int64); taps = np.zeros((h, w), np.int64)
    for ty in (-1, 0, 1):
        for tx in (-1, 0, 1):
            qy, qx = yy + ty, xx + tx
            ry, rx = qy + my, qx + mx
            ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w) & (ry >= 0) & (ry < h) & (rx >= 0) & (rx < w)
            d = cur[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)] - old[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)]
            D += np.where(ok, (d * d).sum(axis=2), 0)
            taps += ok
    qbar = D.astype(np.float64) / (3 * taps).astype(np.float64)
    g = 1.0 / (1.0 + qbar / (sigma * sigma))
    tp = tau * g
    x = np.asarray(x, np.float64).reshape(2, h * w, 3)
    src = ((yy + my) * w + xx + mx).reshape(-1)
    xp = np.asarray(x_prev, np.float64).reshape(2, h * w, 3)[:, src, :]
    t = tp.reshape(1, h * w, 1)
    with np.errstate(invalid="ignore"):
        out = x + t * (xp - x)
    return np.where(np.isnan(xp), x, out), tp


# ---- inputs of the search alone

def motion_case(h, w, seed, kind="random", parent_shape=None):
    """-> (L, Lp, parent or None). kinds: "random" (Lp = a shifted, slightly noisy L: the search has something to find), "noise" (two unrelated maps: many near-ties),
    "equal", "flat" (constant maps: every candidate ties and (0, 0) stays). The parent, if asked for, holds vectors up to +-3: doubled they leave small grids"""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "equal":
        Lp = L.copy()
    elif kind == "flat":
        L = np.full((h, w, 3), 90, np.uint8); Lp = L.copy()
    elif kind == "noise":
        Lp = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        sy, sx = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
        Lp = np.roll(L, (sy, sx), axis=(0, 1))
        Lp = np.clip(Lp.astype(int) + rng.integers(-3, 4, Lp.shape), 0, 255).astype(np.uint8)
    parent = None
    if parent_shape is not None:
        parent = rng.integers(-3, 4, (parent_shape[0], parent_shape[1], 2)).astype(np.int16)
    return L, Lp, parent


def half(n):
    return (n - 1) // 2 + 1


# (grid, kind, with parent, R, penalty): seq_ref.BLEND_CASES' grids at level-0 and refinement settings, odd parent / child sizes (5 -> 9, 6 -> 11), R = 8 at a small
# grid and R = 3 with a parent
MOTION_CASES = [(g, "random", False, 3, 1) for g, _ in seq_ref.BLEND_CASES] + \
               [(g, "noise", True, 1, 0) for g, _ in seq_ref.BLEND_CASES[:5]] + \
               [((9, 9), "random", True, 1, 1), ((9, 11), "noise", True, 1, 3), ((11, 9), "random", True, 3, 1), ((11, 11), "noise", True, 3, 0),
                ((7, 6), "noise", False, 8, 1), ((12, 10), "random", False, 8, 0), ((6, 5), "equal", True, 2, 1), ((8, 8), "flat", True, 2, 255), ((10, 13), "noise", False, 0, 1),
                ((9, 7), "noise", True, 0, 1)]


# ---- the composition

def frame(orc, src, R, ws, bs, state, tau, sigma, mot=None, levels=5, seed=1, bds=2.0, iters=10):
    """seq_ref.frame with rule 4 in place of rule 3 where mot = (radius0, radius, penalty) has a radius > 0. keep gains "motion" per level (zeros where no field is found)"""
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    simg = multi_ref.pyramid(orc, src)
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann = bnn = None
    keep = {k: [] for k in ("result", "ab_nonlocal", "ab_blend", "tau_map", "motion")}
    new_state = []
    out = None
    maxLen = max(H, W, *R["img"].shape[:2])
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    field = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        bh, bw = R["pyr"][l].shape[:2]
        rs = [maxLen // 16, maxLen // 32, maxLen // 64, 32, 32][l]
        rf = R["taps"][4 - l]
        na, nb = orc.feat_normalize(sfeat), orc.feat_normalize(rf)
        if l == 0:
            a0, b0 = orc.nnf_init(ah, aw, bh, bw), orc.nnf_init(bh, bw, ah, aw)
        else:
            a0, b0 = orc.nnf_upsample(ann, ah, aw, bh, bw), orc.nnf_upsample(bnn, bh, bw, ah, aw)
        sab = (seed ^ (0x9E3779B9 * (2 * l + 1))) & 0xffffffff
        sba = (seed ^ (0x9E3779B9 * (2 * l + 2))) & 0xffffffff
        ann, _ = orc.patchmatch(na, nb, a0, iters, rs, sab)
        bnn, _ = orc.patchmatch(nb, na, b0, iters, rs, sba)
        G = orc.bds_vote_image(simg[l], R["pyr"][l], ann, bnn, 1.0, bds)
        E = orc.feature_distance(na, orc.feat_normalize(orc.bds_vote_features(ann, bnn, rf, 1.0, bds)))
        L = orc.bgr2lab(simg[l])
        knn_id, knn_w = orc.knn_graph(L, labels, nl, 1 << l)
        out, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        m = np.zeros((ah, aw, 2), np.int16)
        if tau > 0 and state is not None:
            if on:
                m = field = motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
                Xb, tp = blend_mc(X, state[l][0], L, state[l][1], tau, sigma, m)
            else:
                Xb, tp = seq_ref.blend(X, state[l][0], L, state[l][1], tau, sigma)
            out, _ = fullres_ref.oracle_finish(orc, Xb, ah, aw, H, W, src)
        else:
            Xb, tp = X.copy(), np.zeros((ah, aw))
        new_state.append((Xb, L))
        for name, val in (("result", out), ("ab_nonlocal", X), ("ab_blend", Xb), ("tau_map", tp), ("motion", m)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state


def sequence(orc, frames, ref, ws, bs, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, mot=(RADIUS0, RADIUS, PENALTY), levels=5, **kw):
    """-> (list of results, list of keeps)"""
    R = seq_ref.prepare_reference(orc, ref, ws, bs)
    state, outs, keeps = None, [], []
    for f in frames:
        out, keep, state = frame(orc, f, R, ws, bs, state, tau, sigma, mot=mot, levels=levels, **kw)
        outs.append(out); keeps.append(keep)
    return outs, keeps


# ---- flicker along a known pan

def warped_flicker(outs, srcs, step):
    """seq_ref.pan_frames moves the window `step` px to the right per frame: what frame t shows at x, frame t-1 showed at x + step. -> (flicker, transform flicker)
    taken along that motion on the columns both frames show: mean |o_t(p) - o_(t-1)(p + step)|, and the same on d = out - src"""
    def aligned(a):
        w = a[0].shape[1]
        return float(np.mean([np.abs(a[t][:, :w - step] - a[t - 1][:, step:]).mean() for t in range(1, len(a))]))
    o = [x.astype(np.float64) for x in outs]
    d = [x.astype(np.float64) - s.astype(np.float64) for x, s in zip(outs, srcs)]
    return aligned(o), aligned(d)
