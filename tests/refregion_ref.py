"""Reference region masks (SPEC §6.12) composed from the oracle's exported stages: the pull (rule 2) in numpy with scatter sums, the merge, the level and target masks
and the table rule, and the masked run (one or several references, also at full resolution) as region_ref.run's level loop with the pull inserted. Shared by
tests/test_refregion.py (CPU) and tests/test_gpu_refregion.py. With every Q = 255 the composition is region_ref.run's, bit for bit."""
import numpy as np

import fullres_ref
import multi_ref
import region_ref

PULL_GRIDS = [(1, 1, 1, 1), (4, 4, 3, 4), (9, 11, 7, 5), (56, 64, 48, 60)]          # (ah, aw, bh, bw)


def pull_sums(q, ann, bnn):
    """rule 2's four integer maps on the source's grid: A, ca (coherence: the nine taps of ann) and B, cb (completeness: bnn's source lists) — B1's taps and bounds tests
    on the one-byte image q. Scatter sums: integers carry no order"""
    q = np.ascontiguousarray(q, np.uint8).astype(np.int64)
    ann = np.ascontiguousarray(ann, np.uint32); bnn = np.ascontiguousarray(bnn, np.uint32)
    ah, aw = ann.shape; bh, bw = bnn.shape
    assert q.shape == (bh, bw)
    A, ca, B, cb = (np.zeros(ah * aw, np.int64) for _ in range(4))
    ay, ax = np.mgrid[0:ah, 0:aw]
    by, bx = np.mgrid[0:bh, 0:bw]
    sx, sy = (bnn & 0xFFF).astype(np.int64), ((bnn >> 12) & 0xFFF).astype(np.int64)        # the S pixel each R pixel matches
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            # coherence: the neighbour p + t votes for its match shifted back by t
            nx, ny = ax + dx, ay + dy
            inn = (nx >= 0) & (nx < aw) & (ny >= 0) & (ny < ah)
            v = ann[np.clip(ny, 0, ah - 1), np.clip(nx, 0, aw - 1)]
            xp, yp = (v & 0xFFF).astype(np.int64) - dx, ((v >> 12) & 0xFFF).astype(np.int64) - dy
            ok = inn & (xp >= 0) & (xp < bw) & (yp >= 0) & (yp < bh)
            tgt = (ay * aw + ax)[ok]
            np.add.at(A, tgt, q[yp[ok], xp[ok]])
            np.add.at(ca, tgt, 1)
            # completeness: R pixel r, matched to s, votes r + t onto the target s + t
            tx, ty = sx + dx, sy + dy
            qx, qy = bx + dx, by + dy
            ok = (sx < aw) & (sy < ah) & (tx >= 0) & (tx < aw) & (ty >= 0) & (ty < ah) & (qx >= 0) & (qx < bw) & (qy >= 0) & (qy < bh)
            tgt = (ty * aw + tx)[ok]
            np.add.at(B, tgt, q[qy[ok], qx[ok]])
            np.add.at(cb, tgt, 1)
    return A, ca, B, cb


def pull(q, ann, bnn, w_coh=1.0, w_comp=2.0, rnd=np.rint):
    """rule 2: P = (uint8) rint((A wa + B wb) / (ca wa + cb wb)) in float64 — the products first, then the sums, then the quotient. rnd = np.floor: B1's truncation"""
    ah, aw = np.asarray(ann).shape; bh, bw = np.asarray(bnn).shape
    A, ca, B, cb = pull_sums(q, ann, bnn)
    wa = np.float64(w_coh) / np.float64(aw * ah)
    wb = np.float64(w_comp) / np.float64(bw * bh)
    num = A.astype(np.float64) * wa + B.astype(np.float64) * wb
    den = ca.astype(np.float64) * wa + cb.astype(np.float64) * wb
    return rnd(num / den).astype(np.uint8).reshape(ah, aw)


def merge(lab, pulled):
    """rule 3: P(p) = P_label(p)(p); a reference without a mask (None) counts as 255"""
    lab = np.asarray(lab)
    maps = [np.full(lab.shape, 255, np.uint8) if p is None else p for p in pulled]
    return np.ascontiguousarray(np.choose(lab, maps)) if len(maps) > 1 else maps[0]


def target_mask(orc, P, H, W, ms=None):
    """rule 5: F = resize_u8c1(P -> H x W) (equal sizes: a copy), then the minimum with the source mask at that size where one is set"""
    F = P.copy() if P.shape == (H, W) else region_ref.resize_u8c1(orc, P, H, W)
    return F if ms is None else np.minimum(F, np.ascontiguousarray(ms, np.uint8))


def run(orc, src, m, refs, qs, ws, bs, levels=5, protect=0, form=0, seed=1, bds=2.0, iters=10, full=None, rnd=np.rint):
    """region_ref.run's level loop with the pull behind each masked reference's votes. m: the source mask at src's size or None; qs: per reference its mask or None.
    full = (S0, M0 or None): the last level finishes on the original source S0 with F at S0's size (rule 5; src, m and qs are then the working-size ones).
    -> (result, keep): per level "result", "ab_nonlocal", "ab_mix", "mask" (M_l), "mask_full" (F_l), "p" (P_l), "guide", "err", "label"; "ann" / "bnn" / "ref_mask" /
    "pulled" as [k][l] (the last two None for an unmasked reference)"""
    src = np.ascontiguousarray(src, np.uint8)
    refs = [np.ascontiguousarray(r, np.uint8) for r in refs]
    H, W = src.shape[:2]
    K = len(refs)
    simg = multi_ref.pyramid(orc, src)
    mimg = region_ref.mask_pyramid(orc, m) if m is not None else [None] * 5
    rimg = [multi_ref.pyramid(orc, r) for r in refs]
    qimg = [None if q is None else region_ref.mask_pyramid(orc, q) for q in qs]
    rtap = [orc.vgg19_features(r, ws, bs) for r in refs]
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann, bnn = [None] * K, [None] * K
    keep = {k: [] for k in ("result", "ab_nonlocal", "ab_mix", "mask", "mask_full", "p", "guide", "err", "label")}
    for name in ("ann", "bnn", "ref_mask", "pulled"):
        keep[name] = [[] for _ in range(K)]
    out = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        na = orc.feat_normalize(sfeat)
        guides, errs, pulled = [], [], []
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
            pulled.append(None if qimg[k] is None else pull(qimg[k][l], ann[k], bnn[k], 1.0, bds, rnd))
            keep["ann"][k].append(ann[k]); keep["bnn"][k].append(bnn[k])
            keep["ref_mask"][k].append(None if qimg[k] is None else qimg[k][l]); keep["pulled"][k].append(pulled[k])
        lab = multi_ref.select(errs)
        G, E = multi_ref.merge(lab, guides, errs)
        P = merge(lab, pulled)
        M = P if mimg[l] is None else np.minimum(P, mimg[l])
        knn_id, knn_w = orc.knn_graph(orc.bgr2lab(simg[l]), labels, nl, 1 << l)
        _, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        Xm = region_ref.mix(X, M)
        if full is not None and l == levels - 1:
            S0, M0 = full
            F = target_mask(orc, P, *S0.shape[:2], M0)
            _, fin = fullres_ref.oracle_finish(orc, Xm, ah, aw, H, W, S0, form)
            out = region_ref.compose(orc, S0, fin["lab"], F, protect, form)
        else:
            F = target_mask(orc, P, H, W, m)
            _, fin = fullres_ref.oracle_finish(orc, Xm, ah, aw, H, W, src, form)
            out = region_ref.compose(orc, src, fin["lab"], F, protect, form)
        for name, val in (("result", out), ("ab_nonlocal", X), ("ab_mix", Xm), ("mask", M), ("mask_full", F), ("p", P), ("guide", G), ("err", E), ("label", lab)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep


def pair(orc, src, m, ref, q, ws, bs, **kw):
    """the pair with a source mask m and / or a reference mask q (either None)"""
    return run(orc, src, m, [ref], [q], ws, bs, **kw)


def fullres_pair(orc, src0, m0, ref0, q0, ws, bs, max_side, **kw):
    """rule 5: both images and both masks shrunk by nct_working_size's rule, the masked pair at the working size, the last level's finish and compose on the original"""
    src0 = np.ascontiguousarray(src0, np.uint8); ref0 = np.ascontiguousarray(ref0, np.uint8)
    wh, ww = fullres_ref.working_size(*src0.shape[:2], max_side)
    rh, rw = fullres_ref.working_size(*ref0.shape[:2], max_side)
    shrunk = (wh, ww) != src0.shape[:2]
    src = orc.resize_u8c3(src0, wh, ww) if shrunk else src0
    ref = orc.resize_u8c3(ref0, rh, rw) if (rh, rw) != ref0.shape[:2] else ref0
    m = None if m0 is None else (region_ref.resize_u8c1(orc, m0, wh, ww) if shrunk else np.ascontiguousarray(m0, np.uint8))
    q = None if q0 is None else (region_ref.resize_u8c1(orc, q0, rh, rw) if (rh, rw) != ref0.shape[:2] else np.ascontiguousarray(q0, np.uint8))
    if not shrunk:
        return run(orc, src, m, [ref], [q], ws, bs, **kw)
    return run(orc, src, m, [ref], [q], ws, bs, full=(src0, m0), **kw)


def fit_pixels(keep):
    """rule 7: the pixels nct_pair_fit_lut reads after such a run — the last level's target mask >= 128"""
    return region_ref.kept(keep["mask_full"][-1])


def random_field(seed, ah, aw, bh, bw):
    """a valid random NNF of an ah x aw grid into a bh x bw grid: its taps leave both grids at the borders"""
    rng = np.random.default_rng(seed)
    return ((rng.integers(0, bh, (ah, aw)).astype(np.uint32) << 12) | rng.integers(0, bw, (ah, aw)).astype(np.uint32)).astype(np.uint32)


def collapsed_field(bh, bw, targets):
    """a bnn that sends the R pixels, in raster order and equal shares, onto the given S pixels [(y, x), …]: one target = one list of bh * bw sources"""
    n = bh * bw
    idx = (np.arange(n) * len(targets)) // n
    t = np.asarray(targets, np.uint32)[idx]
    return ((t[:, 0] << 12) | t[:, 1]).astype(np.uint32).reshape(bh, bw)
