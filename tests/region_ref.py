"""Source region masks (SPEC §6.11) composed from the oracle's exported stages: the mask pyramid, the mix, the compose and the masked table fit restated in numpy, the
masked pair (also with several references and at full resolution) as a level loop, and the masks the tests use. Shared by tests/test_region.py (CPU) and
tests/test_gpu_region.py. With M = 255 everywhere the composition is oracle.process_pair bit for bit."""
import numpy as np

import fullres_ref
import lut_ref
import multi_ref
import synth

MASK_KINDS = ("full", "empty", "half", "ramp", "random")
RESIZE_SHAPES = [((57, 57), (29, 29)), ((64, 64), (32, 32)), ((1, 7), (1, 4)), ((5, 1), (3, 1)), ((61, 47), (23, 31))]       # 64 -> 32: the INTER_AREA switch
MIX_SHAPES = [(1, 1), (1, 7), (6, 1), (9, 11), (61, 47)]


def mask(kind, h, w, seed=7):
    """the five masks: all 255, all 0, a slanted binary half-plane, a horizontal ramp that contains every byte value (where w >= 256; else as many as fit), random bytes"""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "empty":
        return np.zeros((h, w), np.uint8)
    if kind == "half":
        return np.where(3 * (xx - w // 2) + (yy - h // 2) > 0, 255, 0).astype(np.uint8)
    if kind == "ramp":
        # R rows share one step of the ramp and split it between them, so that a grid narrower than 256 columns still holds every value it has room for
        R = -(-256 // w)
        return ((xx * R + yy % R) * 256 // (w * R)).astype(np.uint8)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    raise ValueError(kind)


def resize_u8c1(orc, m, dh, dw):
    """rule 1, the definition: channel 0 of the three-channel resize of (M, M, M), the INTER_AREA switch included"""
    m = np.ascontiguousarray(m, np.uint8)
    return np.ascontiguousarray(orc.resize_u8c3(np.repeat(m[:, :, None], 3, axis=2), dh, dw)[:, :, 0])


def _lin_coef(d, ssize, dsize):
    """cv::resize(INTER_LINEAR)'s source index and 11-bit fixed-point weights of destination index d, in float32 as the kernels compute them"""
    f = np.float32((d + 0.5) * (ssize / dsize) - 0.5)
    s = int(np.floor(f))
    f = np.float32(f - np.float32(s))
    if s < 0:
        f, s = np.float32(0), 0
    if s >= ssize - 1:
        f, s = np.float32(0), ssize - 1
    a0 = int(np.int16(np.rint(np.float32(np.float32(1) - f) * np.float32(2048))))
    a1 = int(np.int16(np.rint(f * np.float32(2048))))
    return s, min(s + 1, ssize - 1), a0, a1


def resize_u8c1_np(m, dh, dw):
    """the same resize written out in integers, independent of the oracle: the 2x area case (sum + 2) >> 2, else the fixed-point bilinear chain >>4, *b, >>16, +2, >>2"""
    m = np.ascontiguousarray(m, np.uint8).astype(np.int64)
    sh, sw = m.shape
    if (sh, sw) == (dh, dw):
        return m.astype(np.uint8)
    if sh == 2 * dh and sw == 2 * dw:
        return ((m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    out = np.empty((dh, dw), np.uint8)
    cxs = [_lin_coef(x, sw, dw) for x in range(dw)]
    for y in range(dh):
        y0, y1, b0, b1 = _lin_coef(y, sh, dh)
        for x, (x0, x1, a0, a1) in enumerate(cxs):
            r0 = int(m[y0, x0]) * a0 + int(m[y0, x1]) * a1
            r1 = int(m[y1, x0]) * a0 + int(m[y1, x1]) * a1
            out[y, x] = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
    return out


def mask_pyramid(orc, m):
    """five level masks, coarsest first, each resized from the next finer one like multi_ref.pyramid"""
    lv = [np.ascontiguousarray(m, np.uint8)]
    for _ in range(4):
        h, w = lv[0].shape
        lv.insert(0, resize_u8c1(orc, lv[0], (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return lv


def mix(x, m):
    """rule 2 in float64, operation for operation: x [2][h*w][3], m [h][w] bytes -> X'. M = 255 copies the words, M = 0 writes the identity transform"""
    x = np.ascontiguousarray(x, np.float64).reshape(2, -1, 3)
    M = np.ascontiguousarray(m, np.uint8).reshape(-1, 1)
    f = M.astype(np.float64) / 255.0
    with np.errstate(invalid="ignore"):
        a = 1.0 + f * (x[0] - 1.0)
        b = f * x[1]
    a = np.where(M == 255, x[0], np.where(M == 0, 1.0, a))
    b = np.where(M == 255, x[1], np.where(M == 0, 0.0, b))
    return np.stack([a, b])


def keep_map(lab_s, lab_o, m, protect):
    """rule 3's keep(p)"""
    same = (np.asarray(lab_o) == np.asarray(lab_s)).all(axis=-1)
    m = np.asarray(m, np.uint8).reshape(same.shape)
    return (bool(protect) & (m == 0)) | ((m != 255) & same)


def compose(orc, s_bgr, lab_o, m, protect=0, form=None):
    """rule 3: out = keep ? S : Lab2BGR(Lab_o), at the size of s_bgr with the mask at that size"""
    s = np.ascontiguousarray(s_bgr, np.uint8)
    lab_o = np.ascontiguousarray(lab_o, np.uint8).reshape(s.shape)
    k = keep_map(orc.bgr2lab(s), lab_o, m, protect)
    return np.where(k[..., None], s, orc.lab2bgr(lab_o, form))


def kept(m):
    """rule 7: the pixels a masked fit reads"""
    return np.asarray(m, np.uint8).reshape(-1) >= 128


def splat(src, res, m, N):
    k = kept(m)
    return lut_ref.splat(np.asarray(src, np.uint8).reshape(-1, 3)[k], np.asarray(res, np.uint8).reshape(-1, 3)[k], N)


def run(orc, src, m, refs, ws, bs, levels=5, protect=0, form=0, seed=1, bds=2.0, iters=10, full=None):
    """the level loop of multi_ref.multi (K = 1: seq_ref.frame's) with the mix between S1 and the finish and the compose behind it. m: the mask at src's size.
    full = (S0, M0): the last level finishes on the original source S0 and composes with M0 (rule 5; src and m are then the working-size ones).
    -> (result, keep): per level "result", "ab_nonlocal", "ab_mix", "mask", "guide", "err", "label", and "ann" / "bnn" as [k][l]"""
    src = np.ascontiguousarray(src, np.uint8)
    refs = [np.ascontiguousarray(r, np.uint8) for r in refs]
    H, W = src.shape[:2]
    K = len(refs)
    simg = multi_ref.pyramid(orc, src)
    mimg = mask_pyramid(orc, m)
    rimg = [multi_ref.pyramid(orc, r) for r in refs]
    rtap = [orc.vgg19_features(r, ws, bs) for r in refs]
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann, bnn = [None] * K, [None] * K
    keep = {k: [] for k in ("result", "ab_nonlocal", "ab_mix", "mask", "guide", "err", "label")}
    keep["ann"], keep["bnn"] = [[] for _ in range(K)], [[] for _ in range(K)]
    out = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        na = orc.feat_normalize(sfeat)
        guides, errs = [], []
        for k in range(K):
            bh, bw = rimg[k][l].shape[:2]
            maxLen = max(H, W, *refs[k].shape[:2])
            rs = [maxLen // 16, maxLen // 32, maxLen // 64, 32, 32][l]
            rf = rtap[k][4 - l]
            nb = orc.feat_normalize(rf)
            if l == 0:
                a0, b0 = orc.nnf_init(ah, aw, bh, bw), orc.nnf_init(bh, bw, ah, aw)
            else:
                a0, b0 = orc.nnf_upsample(ann[k], ah, aw, bh, bw), orc.nnf_upsample(bnn[k], bh, bw, ah, aw)
            sab = (seed ^ (0x9E3779B9 * (2 * l + 1))) & 0xffffffff
            sba = (seed ^ (0x9E3779B9 * (2 * l + 2))) & 0xffffffff
            ann[k], _ = orc.patchmatch(na, nb, a0, iters, rs, sab)
            bnn[k], _ = orc.patchmatch(nb, na, b0, iters, rs, sba)
            guides.append(orc.bds_vote_image(simg[l], rimg[k][l], ann[k], bnn[k], 1.0, bds))
            errs.append(orc.feature_distance(na, orc.feat_normalize(orc.bds_vote_features(ann[k], bnn[k], rf, 1.0, bds))))
            keep["ann"][k].append(ann[k]); keep["bnn"][k].append(bnn[k])
        lab = multi_ref.select(errs)
        G, E = multi_ref.merge(lab, guides, errs)
        knn_id, knn_w = orc.knn_graph(orc.bgr2lab(simg[l]), labels, nl, 1 << l)
        _, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        Xm = mix(X, mimg[l])
        if full is not None and l == levels - 1:
            S0, M0 = full
            _, fin = fullres_ref.oracle_finish(orc, Xm, ah, aw, H, W, S0, form)
            out = compose(orc, S0, fin["lab"], M0, protect, form)
        else:
            _, fin = fullres_ref.oracle_finish(orc, Xm, ah, aw, H, W, src, form)
            out = compose(orc, src, fin["lab"], m, protect, form)
        for name, val in (("result", out), ("ab_nonlocal", X), ("ab_mix", Xm), ("mask", mimg[l]), ("guide", G), ("err", E), ("label", lab)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep


def pair(orc, src, m, ref, ws, bs, **kw):
    """the masked pair: run() with one reference"""
    return run(orc, src, m, [ref], ws, bs, **kw)


def fullres_pair(orc, src0, m0, ref0, ws, bs, max_side, **kw):
    """rule 5: both images and the mask shrunk by nct_working_size's rule, the masked pair at the working size, the last level's finish and compose on the originals"""
    src0 = np.ascontiguousarray(src0, np.uint8); ref0 = np.ascontiguousarray(ref0, np.uint8)
    wh, ww = fullres_ref.working_size(*src0.shape[:2], max_side)
    rh, rw = fullres_ref.working_size(*ref0.shape[:2], max_side)
    src = orc.resize_u8c3(src0, wh, ww) if (wh, ww) != src0.shape[:2] else src0
    ref = orc.resize_u8c3(ref0, rh, rw) if (rh, rw) != ref0.shape[:2] else ref0
    m = resize_u8c1(orc, m0, wh, ww) if (wh, ww) != src0.shape[:2] else np.ascontiguousarray(m0, np.uint8)
    if (wh, ww) == src0.shape[:2]:
        return run(orc, src, m, [ref], ws, bs, **kw)
    return run(orc, src, m, [ref], ws, bs, full=(src0, m0), **kw)


def mix_case(h, w, kind, seed=3):
    """inputs of the mix alone: coefficients of the scale S1 returns, one of the five masks, and NaNs in a, in b, under M = 0 and under M = 255"""
    rng = np.random.default_rng(seed + h * 131 + w)
    n = h * w
    x = np.stack([1.0 + 0.3 * rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3))])
    m = mask(kind, h, w, seed)
    return x, m


def with_nans(x, m):
    """NaN in a at a partial pixel, in b at another, one under M = 0 and one under M = 255 (the mask is edited to hold those values where the grid has room)"""
    x = x.copy(); shape = m.shape; m = m.copy().reshape(-1)
    n = m.size
    spots = [(0, 0, 77), (1, (n // 2) % n, 130), (0, (n - 1) % n, 0), (1, (n // 3) % n, 255)]
    for part, i, val in spots:
        m[i] = val
    for part, i, val in spots:
        x[part, i, 1] = np.nan
    return x, m.reshape(shape)


def compose_case(orc, h, w, seed=5):
    """a source, a Lab result and a mask such that each of M = 0, M in 1 … 254 and M = 255 holds pixels with Lab_o == Lab_S and pixels without"""
    rng = np.random.default_rng(seed)
    s = synth.image(seed, h, w)
    lab_s = orc.bgr2lab(s)
    lab_o = np.clip(lab_s.astype(int) + rng.integers(-9, 10, lab_s.shape), 0, 255).astype(np.uint8)
    same = rng.random((h, w)) < 0.3
    lab_o[same] = lab_s[same]
    m = rng.integers(0, 256, (h, w), dtype=np.uint8)
    m[rng.random((h, w)) < 0.25] = 0
    m[rng.random((h, w)) < 0.25] = 255
    return s, lab_s, lab_o, m


def compose_shares(lab_s, lab_o, m):
    """the share of all pixels that have Lab_o == Lab_S with M == 0, with M in 1 … 254 and with M == 255"""
    same = (lab_o == lab_s).all(axis=-1)
    return [float((same & c).mean()) for c in (m == 0, (m != 0) & (m != 255), m == 255)]
