"""Frame sequences (SPEC §6.3) composed from the oracle's exported stages, the blend rule restated in numpy, and the synthetic sequences the flicker figures are
taken on. Shared by tests/test_seq.py (CPU) and tests/test_gpu_seq.py. Frame 0 and every frame with tau = 0 of the composition are oracle.process_pair bit for bit."""
import numpy as np

import fullres_ref
import multi_ref
import synth

TAU, SIGMA = 0.7, 10.0           # nct_seq_params_default


def blend(x, x_prev, lab, lab_prev, tau, sigma):
    """SPEC §6.3 rule 3 in numpy float64, operation for operation: x, x_prev [2][h*w][3]; lab, lab_prev h x w x 3 uint8 -> (X' [2][h*w][3], tau_p [h][w])"""
    lab = np.asarray(lab, np.uint8)
    h, w = lab.shape[:2]
    d = lab.astype(np.int64) - np.asarray(lab_prev, np.uint8).astype(np.int64)
    sq = np.pad((d * d).sum(axis=2), 1)                 # a tap outside the grid adds 0 = is skipped
    inside = np.pad(np.ones((h, w), np.int64), 1)
    D = np.zeros((h, w), np.int64)
    taps = np.zeros((h, w), np.int64)
    for dy in range(3):
        for dx in range(3):
            D += sq[dy:dy + h, dx:dx + w]
            taps += inside[dy:dy + h, dx:dx + w]
    qbar = D.astype(np.float64) / (3 * taps).astype(np.float64)
    g = 1.0 / (1.0 + qbar / (sigma * sigma))
    tp = tau * g
    x = np.asarray(x, np.float64).reshape(2, h * w, 3)
    xp = np.asarray(x_prev, np.float64).reshape(2, h * w, 3)
    t = tp.reshape(1, h * w, 1)
    with np.errstate(invalid="ignore"):
        out = x + t * (xp - x)
    return np.where(np.isnan(xp), x, out), tp


# ---- inputs of the blend alone: shared by the CPU test of the numpy rule and the GPU test of the kernel

def blend_case(h, w, seed, kind="random"):
    rng = np.random.default_rng(seed)
    n = h * w
    x = np.stack([1.0 + 0.3 * rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3))])
    xp = np.stack([1.0 + 0.3 * rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3))])
    lab = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "equal":
        labp = lab.copy()
    elif kind == "extreme":                                    # the largest D: every byte differs by 255
        lab = np.zeros((h, w, 3), np.uint8); labp = np.full((h, w, 3), 255, np.uint8)
    else:                                                      # small differences in most places, a large one in a patch
        labp = np.clip(lab.astype(int) + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
        labp[h // 3:h // 3 + max(1, h // 4), w // 3:w // 3 + max(1, w // 4)] = rng.integers(0, 256, 3, dtype=np.uint8)
    if kind == "nan_prev":
        xp.reshape(-1)[::5] = np.nan
    if kind == "nan_x":
        x.reshape(-1)[::7] = np.nan
    if kind == "nan_both":
        xp.reshape(-1)[::5] = np.nan; x.reshape(-1)[::7] = np.nan
    return x, xp, lab, labp


BLEND_CASES = [((1, 1), "random"), ((1, 7), "random"), ((6, 1), "random"), ((5, 4), "random"), ((9, 11), "random"), ((7, 5), "equal"), ((4, 6), "extreme"),
               ((6, 7), "nan_prev"), ((6, 7), "nan_x"), ((5, 8), "nan_both")]


def prepare_reference(orc, ref, ws, bs):
    """what nct_seq_begin computes once: the reference's pyramid and its five taps"""
    ref = np.ascontiguousarray(ref, np.uint8)
    return {"img": ref, "pyr": multi_ref.pyramid(orc, ref), "taps": orc.vgg19_features(ref, ws, bs)}


def frame(orc, src, R, ws, bs, state, tau, sigma, levels=5, seed=1, bds=2.0, iters=10):
    """one frame: the level loop of multi_ref.multi for one reference with rule 3 between S1 and the finish. state: None (a first frame) or the list per level of
    (X', L) the previous frame returned. -> (result, keep, new state); keep: per level "result", "ab_nonlocal", "ab_blend", "tau_map" """
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    simg = multi_ref.pyramid(orc, src)
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann = bnn = None
    keep = {k: [] for k in ("result", "ab_nonlocal", "ab_blend", "tau_map")}
    new_state = []
    out = None
    maxLen = max(H, W, *R["img"].shape[:2])
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
        if tau > 0 and state is not None:
            Xb, tp = blend(X, state[l][0], L, state[l][1], tau, sigma)
            out, _ = fullres_ref.oracle_finish(orc, Xb, ah, aw, H, W, src)
        else:
            Xb, tp = X.copy(), np.zeros((ah, aw))
        new_state.append((Xb, L))
        for name, val in (("result", out), ("ab_nonlocal", X), ("ab_blend", Xb), ("tau_map", tp)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state


def sequence(orc, frames, ref, ws, bs, tau=TAU, sigma=SIGMA, levels=5, **kw):
    """-> (list of results, list of keeps)"""
    R = prepare_reference(orc, ref, ws, bs)
    state, outs, keeps = None, [], []
    for f in frames:
        out, keep, state = frame(orc, f, R, ws, bs, state, tau, sigma, levels=levels, **kw)
        outs.append(out); keeps.append(keep)
    return outs, keeps


def _noisy(img, rng, noise):
    return np.clip(np.rint(img.astype(np.float64) + rng.normal(0.0, noise, img.shape)), 0, 255).astype(np.uint8)


def static_frames(n, h, w, seed=1000, noise=2.0, rng_seed=5):
    """one synth image under fresh sensor-like noise (sigma = `noise` grey levels) per frame"""
    rng = np.random.default_rng(rng_seed)
    base = synth.image(seed, h, w)
    return [_noisy(base, rng, noise) for _ in range(n)]


def pan_frames(n, h, w, seed=1000, noise=2.0, rng_seed=5, step=1):
    """a window that moves `step` px per frame across a wider synth image, plus the same noise"""
    rng = np.random.default_rng(rng_seed)
    base = synth.image(seed, h, w + step * (n - 1))
    return [_noisy(base[:, step * t:step * t + w], rng, noise) for t in range(n)]


def flicker(outs):
    """mean |out_t - out_(t-1)| in grey levels"""
    return float(np.mean([np.abs(outs[t].astype(np.float64) - outs[t - 1].astype(np.float64)).mean() for t in range(1, len(outs))]))


def transform_flicker(outs, srcs):
    """the same on out - src: the source's own noise and motion removed"""
    d = [o.astype(np.float64) - s.astype(np.float64) for o, s in zip(outs, srcs)]
    return float(np.mean([np.abs(d[t] - d[t - 1]).mean() for t in range(1, len(d))]))
