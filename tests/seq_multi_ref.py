"""Frame sequences over several references with a held selection (SPEC §6.18): rules 1-6 and the label carry restated in numpy, inside the composition of
tests/multi_ref.py (the correspondences per reference, the merge) and tests/seq_ref.py / seq_mc_ref.py / seq_prop_ref.py (the blend, the field, the propagated frame);
the inputs of the rule alone; and the fixtures and the flip measure of the quality statement. Shared by tests/test_seq_multi.py (CPU) and tests/test_gpu_seq_multi.py.
All double arithmetic is the rule's, operation for operation; with one reference the composition is seq_mc_ref.frame's."""
import numpy as np

import fullres_ref
import multi_ref
import seq_mc_ref
import seq_prop_ref
import seq_ref
import synth

HOLD = 0.005                    # nct_seq_hold_default (the sweep that chose it)
HOLDS = (0.0, 0.005, 0.01, 0.02, 0.05, 0.1)


def scores(errs):
    """rule 1 / §6.2 rule 2 -> (score [K][h][w] float64, n [h][w] int64: the window taps inside the grid)"""
    K = len(errs)
    h, w = errs[0].shape
    sc = np.empty((K, h, w))
    for k in range(K):
        e = np.asarray(errs[k], np.float32).astype(np.float64)
        p = np.pad(np.where(np.isnan(e), 0.0, e), 1)           # a tap outside the grid adds +0.0 = is skipped
        acc = np.zeros((h, w))
        for dy in range(3):
            for dx in range(3):
                acc = acc + p[dy:dy + h, dx:dx + w]
        sc[k] = acc
    inside = np.pad(np.ones((h, w), np.int64), 1)
    n = sum(inside[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return sc, n


def free_label(sc):
    """the lowest k of the smallest score, by strict comparisons in index order"""
    f = np.zeros(sc.shape[1:], np.int64)
    best = sc[0].copy()
    for k in range(1, sc.shape[0]):
        take = sc[k] < best
        f = np.where(take, k, f); best = np.where(take, sc[k], best)
    return f, best


def clamped(field, h, w):
    """rule 2: the field's vectors clamped component-wise so that p + m is inside the grid; None: zeros -> (my, mx) int64 [h][w]"""
    if field is None:
        return np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    f = np.asarray(field, np.int16).astype(np.int64).reshape(h, w, 2)
    return np.clip(yy + f[..., 0], 0, h - 1) - yy, np.clip(xx + f[..., 1], 0, w - 1) - xx


def gain(lab, lab_prev, field, sigma):
    """rule 3: the g of seq_ref.blend (field None) / seq_mc_ref.blend_mc, operation for operation -> float64 [h][w]"""
    lab = np.asarray(lab, np.uint8)
    h, w = lab.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    my, mx = clamped(field, h, w)
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
    return 1.0 / (1.0 + qbar / (sigma * sigma))


def carry(label_prev, field):
    """rule 7: label_prev read at p + m(p), the vector clamped first; None: the map as it is"""
    lp = np.asarray(label_prev, np.uint8)
    h, w = lp.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    my, mx = clamped(field, h, w)
    return np.ascontiguousarray(lp[yy + my, xx + mx])


def select_hold(errs, prev_label, lab, lab_prev, field, hold, sigma):
    """rules 1-5 -> (label uint8 [h][w], free label uint8 [h][w], margin float64 [h][w])"""
    K = len(errs)
    sc, n = scores(errs)
    f, score_f = free_label(sc)
    j = carry(prev_label, field).astype(np.int64)
    g = gain(lab, lab_prev, field, sigma)
    margin = (hold * g) * n.astype(np.float64)
    score_j = np.take_along_axis(sc, np.minimum(j, K - 1)[None], axis=0)[0]
    free = (j >= K) | (score_f < score_j - margin)
    return np.where(free, f, j).astype(np.uint8), f.astype(np.uint8), margin


def select_hold_scalar(errs, prev_label, lab, lab_prev, field, hold, sigma):
    """the same, one pixel at a time in python floats (IEEE double): what the numpy rule is pinned to"""
    K = len(errs)
    h, w = errs[0].shape
    label = np.zeros((h, w), np.uint8); free = np.zeros((h, w), np.uint8); margin = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            my = mx = 0
            if field is not None:
                my = min(max(y + int(field[y][x][0]), 0), h - 1) - y; mx = min(max(x + int(field[y][x][1]), 0), w - 1) - x
            sc, n = [0.0] * K, 0
            D = taps = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < h and 0 <= qx < w):
                        continue
                    n += 1
                    for k in range(K):
                        v = float(np.float32(errs[k][qy][qx]))
                        sc[k] = sc[k] + (0.0 if v != v else v)
                    ry, rx = qy + my, qx + mx
                    if 0 <= ry < h and 0 <= rx < w:
                        taps += 1
                        D += sum((int(lab[qy][qx][c]) - int(lab_prev[ry][rx][c])) ** 2 for c in range(3))
            f = 0
            for k in range(1, K):
                if sc[k] < sc[f]:
                    f = k
            j = int(prev_label[y + my][x + mx])
            qbar = float(D) / float(3 * taps)
            g = 1.0 / (1.0 + qbar / (sigma * sigma))
            mg = (hold * g) * float(n)
            free[y][x] = f; margin[y][x] = mg
            label[y][x] = f if (j >= K or sc[f] < sc[j] - mg) else j
    return label, free, margin


# ---- inputs of the rule alone: shared by the CPU test of the numpy rule and the GPU test of the kernel

def hold_case(h, w, K, seed, kind="random", with_field=True):
    """-> dict(errs, guides, prev_label, lab, lab_prev, field). kinds: "random" (smooth error maps whose differences are of the order of the margins, Lab maps that agree
    in most places), "ties" (every map the same words: f = 0 everywhere, a kept label stays), "nan" (NaN words in every map), "stale" (kept labels >= K among the valid
    ones), "far" (vectors up to +-9: most leave small grids)"""
    rng = np.random.default_rng(seed)
    base = -0.6 + 0.05 * rng.standard_normal((h, w))
    errs = [(base + 0.01 * rng.standard_normal((h, w))).astype(np.float32) for _ in range(K)]
    if kind == "ties":
        errs = [errs[0].copy() for _ in range(K)]
    if kind == "nan":
        for k in range(K):
            errs[k].reshape(-1)[k::3] = np.nan
    guides = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(K)]
    prev = rng.integers(0, K, (h, w), dtype=np.uint8)
    if kind == "stale":
        prev.reshape(-1)[::2] = rng.integers(K, 256, prev.reshape(-1)[::2].shape, dtype=np.uint8)
    lab = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    labp = np.clip(lab.astype(int) + rng.integers(-4, 5, (h, w, 3)), 0, 255).astype(np.uint8)
    labp[h // 3:h // 3 + max(1, h // 4), w // 3:w // 3 + max(1, w // 4)] = rng.integers(0, 256, 3, dtype=np.uint8)
    r = 9 if kind == "far" else 3
    field = rng.integers(-r, r + 1, (h, w, 2)).astype(np.int16) if with_field else None
    return dict(errs=errs, guides=guides, prev_label=prev, lab=lab, lab_prev=labp, field=field)


KINDS = ("random", "ties", "nan", "stale", "far")


# ---- the composition

def prepare_references(orc, refs, ws, bs):
    return [seq_ref.prepare_reference(orc, r, ws, bs) for r in refs]


def frame(orc, src, Rs, ws, bs, state, tau, sigma, hold, mot=None, levels=5, seed=1, bds=2.0, iters=10):
    """one full frame over the references Rs (prepare_references): multi_ref.multi's level loop, the selection of SPEC §6.18 in the place of multi_ref.select, and
    seq_mc_ref.frame's blend between S1 and the finish. state: None (a first frame) or the list per level of (X', L, labels) the previous frame returned.
    -> (result, keep, new state); keep per level: "ref_err" and "ref_guide" as [k][l]; "free_label", "margin", "label", "guide", "err", "ab_nonlocal", "ab_blend", "tau_map",
    "motion", "result" as [l]"""
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    K = len(Rs)
    simg = multi_ref.pyramid(orc, src)
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann, bnn = [None] * K, [None] * K
    keep = {k: [[] for _ in range(K)] for k in ("ref_err", "ref_guide")}
    keep.update({k: [] for k in ("free_label", "margin", "label", "guide", "err", "ab_nonlocal", "ab_blend", "tau_map", "motion", "result")})
    new_state = []
    out = None
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    blends = tau > 0 and state is not None
    field = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        na = orc.feat_normalize(sfeat)
        guides, errs = [], []
        for k in range(K):
            R = Rs[k]
            bh, bw = R["pyr"][l].shape[:2]
            maxLen = max(H, W, *R["img"].shape[:2])
            rs = [maxLen // 16, maxLen // 32, maxLen // 64, 32, 32][l]
            rf = R["taps"][4 - l]
            nb = orc.feat_normalize(rf)
            if l == 0:
                a0, b0 = orc.nnf_init(ah, aw, bh, bw), orc.nnf_init(bh, bw, ah, aw)
            else:
                a0, b0 = orc.nnf_upsample(ann[k], ah, aw, bh, bw), orc.nnf_upsample(bnn[k], bh, bw, ah, aw)
            sab = (seed ^ (0x9E3779B9 * (2 * l + 1))) & 0xffffffff
            sba = (seed ^ (0x9E3779B9 * (2 * l + 2))) & 0xffffffff
            ann[k], _ = orc.patchmatch(na, nb, a0, iters, rs, sab)
            bnn[k], _ = orc.patchmatch(nb, na, b0, iters, rs, sba)
            guides.append(orc.bds_vote_image(simg[l], R["pyr"][l], ann[k], bnn[k], 1.0, bds))
            errs.append(orc.feature_distance(na, orc.feat_normalize(orc.bds_vote_features(ann[k], bnn[k], rf, 1.0, bds))))
            keep["ref_err"][k].append(errs[-1]); keep["ref_guide"][k].append(guides[-1])
        L = orc.bgr2lab(simg[l])
        m = np.zeros((ah, aw, 2), np.int16)
        if blends and on:
            m = field = seq_mc_ref.motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
        if K == 1:
            lab = free = np.zeros((ah, aw), np.uint8); margin = np.zeros((ah, aw))
        elif blends and hold > 0:
            lab, free, margin = select_hold(errs, state[l][2], L, state[l][1], m if on else None, hold, sigma)
        else:
            lab = free = multi_ref.select(errs); margin = np.zeros((ah, aw))
        G, E = multi_ref.merge(lab, guides, errs)
        knn_id, knn_w = orc.knn_graph(L, labels, nl, 1 << l)
        out, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        if blends:
            Xb, tp = seq_mc_ref.blend_mc(X, state[l][0], L, state[l][1], tau, sigma, m if on else None)
            out, _ = fullres_ref.oracle_finish(orc, Xb, ah, aw, H, W, src)
        else:
            Xb, tp = X.copy(), np.zeros((ah, aw))
        new_state.append((Xb, L, lab))
        for name, val in (("free_label", free), ("margin", margin), ("label", lab), ("guide", G), ("err", E), ("ab_nonlocal", X), ("ab_blend", Xb), ("tau_map", tp),
                          ("motion", m), ("result", out)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state


def frame_propagate(orc, src, state, mot=None, levels=5):
    """seq_prop_ref.frame_propagate, and the kept labels carried along the fields it found (motion off: left as they are)"""
    out, keep, st = seq_prop_ref.frame_propagate(orc, src, state, mot=mot, levels=levels)
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    new_state = [(st[l][0], st[l][1], carry(state[l][2], keep["motion"][l] if on else None)) for l in range(levels)]
    keep["label"] = [s[2] for s in new_state]
    return out, keep, new_state


def sequence(orc, frames, refs, ws, bs, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, hold=HOLD, mot=(seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY), levels=5, full=None, **kw):
    """full: None (every frame is a full frame) or a list of booleans, False = a propagated frame -> (list of results, list of keeps)"""
    Rs = prepare_references(orc, refs, ws, bs)
    state, outs, keeps = None, [], []
    for t, f in enumerate(frames):
        if full is None or full[t]:
            out, keep, state = frame(orc, f, Rs, ws, bs, state, tau, sigma, hold, mot=mot, levels=levels, **kw)
        else:
            out, keep, state = frame_propagate(orc, f, state, mot=mot, levels=levels)
        outs.append(out); keeps.append(keep)
    return outs, keeps


# ---- the quality statement: two fixtures and the flip share along the motion

QSIZE = (64, 56)


def competing(a, seed=77):
    """a reference that competes with `a`: its copy under a small global colour cast and fresh noise. The two matching errors differ by little almost everywhere,
    so the free selection's labels follow the frame's noise"""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(a.astype(np.float64) * 0.97 + 4.0 + rng.normal(0.0, 2.0, a.shape)), 0, 255).astype(np.uint8)


def quality_references():
    a = synth.image(1001, 48, 64)
    return [a, competing(a)]


def quality_frames(kind, n=2):
    h, w = QSIZE
    return seq_ref.static_frames(n, h, w) if kind == "static" else seq_ref.pan_frames(n, h, w, step=4)


def flip_share(keeps, level=-1):
    """the share of pixels of a level (default: the last one run) with l_t(p) != l_(t-1)(p + m(p)), m the field the frame found, over the frames after the first"""
    flips = []
    for t in range(1, len(keeps)):
        prev = keeps[t - 1]["label"][level]
        flips.append(float((keeps[t]["label"][level] != carry(prev, keeps[t]["motion"][level])).mean()))
    return float(np.mean(flips))
