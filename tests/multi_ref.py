"""Colour transfer from several references (SPEC §6.2) composed from the oracle's exported stages, and the selection rule restated in numpy.
Shared by tests/test_multi_ref.py (CPU) and tests/test_gpu_multi_ref.py. With one reference the composition is oracle.process_pair bit for bit."""
import numpy as np

MAX_REFS = 8


def select(errs):
    """SPEC §6.2 rule 2: per pixel the lowest k whose 3 x 3 sum of E_k (double, dy outer / dx inner, NaN = 0.0, taps outside the grid skipped) is smallest -> uint8 labels"""
    K = len(errs)
    h, w = errs[0].shape
    sc = np.empty((K, h, w))
    for k in range(K):
        e = errs[k].astype(np.float64)
        e = np.where(np.isnan(e), 0.0, e)
        p = np.pad(e, 1)                            # a tap outside the grid adds +0.0 = is skipped
        acc = np.zeros((h, w))
        for dy in range(3):
            for dx in range(3):
                acc = acc + p[dy:dy + h, dx:dx + w]
        sc[k] = acc
    return np.argmin(sc, axis=0).astype(np.uint8)   # first minimum = lowest index


def merge(lab, guides, errs):
    """rule 3: G(p) = G_l(p)(p), E(p) = E_l(p)(p) — the fp32 word, NaN included"""
    G = np.choose(lab[..., None], guides)
    E = np.choose(lab, [e.view(np.uint32) for e in errs]).view(np.float32)
    return np.ascontiguousarray(G), np.ascontiguousarray(E)


def pyramid(orc, img):
    """five levels, coarsest first, each the bilinear shrink of the next finer one to ((h-1)//2+1, (w-1)//2+1) (main.cu:104-108)"""
    lv = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(4):
        h, w = lv[0].shape[:2]
        lv.insert(0, orc.resize_u8c3(lv[0], (h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return lv


def multi(orc, src, refs, ws, bs, levels=5, seed=1, bds=2.0, iters=10, lab2bgr_form=0):
    """-> (result, per-level dict): "ann", "bnn", "annd", "bnnd", "ref_guide", "ref_err" as [k][l]; "label", "guide", "err", "result" as [l] (levels that ran)"""
    src = np.ascontiguousarray(src, np.uint8)
    refs = [np.ascontiguousarray(r, np.uint8) for r in refs]
    H, W = src.shape[:2]
    K = len(refs)
    assert 1 <= K <= MAX_REFS
    simg = pyramid(orc, src)
    rimg = [pyramid(orc, r) for r in refs]
    rtap = [orc.vgg19_features(r, ws, bs) for r in refs]            # tap t belongs to level 4 - t
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann = [None] * K
    bnn = [None] * K
    keep = {k: [[] for _ in range(K)] for k in ("ann", "bnn", "annd", "bnnd", "ref_guide", "ref_err")}
    keep.update({k: [] for k in ("label", "guide", "err", "result")})
    out = None
    form_before = orc.l.orc_get_lab2bgr_form()
    orc.l.orc_set_lab2bgr_form(lab2bgr_form)
    try:
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
                ann[k], annd = orc.patchmatch(na, nb, a0, iters, rs, sab)
                bnn[k], bnnd = orc.patchmatch(nb, na, b0, iters, rs, sba)
                guides.append(orc.bds_vote_image(simg[l], rimg[k][l], ann[k], bnn[k], 1.0, bds))
                v = orc.bds_vote_features(ann[k], bnn[k], rf, 1.0, bds)
                errs.append(orc.feature_distance(na, orc.feat_normalize(v)))
                for name, val in (("ann", ann[k]), ("bnn", bnn[k]), ("annd", annd), ("bnnd", bnnd), ("ref_guide", guides[-1]), ("ref_err", errs[-1])):
                    keep[name][k].append(val)
            lab = select(errs)
            G, E = merge(lab, guides, errs)
            knn_id, knn_w = orc.knn_graph(orc.bgr2lab(simg[l]), labels, nl, 1 << l)
            out = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l)
            for name, val in (("label", lab), ("guide", G), ("err", E), ("result", out)):
                keep[name].append(val)
            if l < levels - 1:
                sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    finally:
        orc.l.orc_set_lab2bgr_form(form_before)
    return out, keep


def shares(lab, K):
    """fraction of the label map each reference holds"""
    return [float((lab == k).mean()) for k in range(K)]
