"""Reference region masks in sequences (SPEC §6.19): rule 3's hold of the pulled mask restated in numpy, inside the composition of tests/seq_multi_ref.py (the
correspondences per reference, the held selection, the blend, the carry), tests/refregion_ref.py (the pull, the merge, the target mask), tests/seq_region_ref.py (the
out-of-place mix and the finishes of a masked sequence frame), tests/region_ref.py, tests/seq_prop_ref.py, tests/seq_mc_ref.py and tests/fullres_ref.py. The only new
arithmetic is pull_hold. Shared by tests/test_seq_refregion.py (CPU) and tests/test_gpu_seq_refregion.py. The state a frame returns is never mixed."""
import numpy as np

import fullres_ref
import multi_ref
import refregion_ref
import region_ref
import seq_mc_ref
import seq_multi_ref
import seq_prop_ref
import seq_ref
import seq_region_ref

KINDS = "FBPB"                   # the frame kinds of the tests' plan: full (first), blended, propagated, blended
GRIDS = [(1, 1), (1, 7), (6, 1), (9, 11), (17, 16), (61, 47)]


def pull_hold(pulled, label, prev, lab, lab_prev, field, src_mask, tau, sigma):
    """rules 2-4 -> (P' uint8 [h][w], M uint8 [h][w], the free P uint8 [h][w]). pulled: K maps or None (= 255); label None: reference 0"""
    prev = np.asarray(prev, np.uint8)
    lab_map = np.zeros(prev.shape, np.int64) if label is None else np.asarray(label).astype(np.int64)
    P = refregion_ref.merge(lab_map, [None if p is None else np.asarray(p, np.uint8) for p in pulled])
    j = seq_multi_ref.carry(prev, field).astype(np.float64)
    tp = tau * seq_multi_ref.gain(lab, lab_prev, field, sigma)
    Pf = P.astype(np.float64)
    held = np.rint(Pf + tp * (j - Pf)).astype(np.uint8)
    M = held if src_mask is None else np.minimum(held, np.asarray(src_mask, np.uint8))
    return held, M, np.ascontiguousarray(P)


def pull_hold_scalar(pulled, label, prev, lab, lab_prev, field, src_mask, tau, sigma):
    """the same, one pixel at a time in python floats (IEEE double): what the numpy rule is pinned to"""
    h, w = np.asarray(prev).shape
    held = np.zeros((h, w), np.uint8); M = np.zeros((h, w), np.uint8); free = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            my = mx = 0
            if field is not None:
                my = min(max(y + int(field[y][x][0]), 0), h - 1) - y; mx = min(max(x + int(field[y][x][1]), 0), w - 1) - x
            D = taps = 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = y + dy, x + dx
                    ry, rx = qy + my, qx + mx
                    if 0 <= qy < h and 0 <= qx < w and 0 <= ry < h and 0 <= rx < w:
                        taps += 1
                        D += sum((int(lab[qy][qx][c]) - int(lab_prev[ry][rx][c])) ** 2 for c in range(3))
            k = 0 if label is None else int(label[y][x])
            P = 255 if pulled[k] is None else int(pulled[k][y][x])
            j = int(prev[y + my][x + mx])
            qbar = float(D) / float(3 * taps)
            g = 1.0 / (1.0 + qbar / (sigma * sigma))
            tp = tau * g
            v = float(P) + tp * (float(j) - float(P))
            r = int(np.rint(v))                                 # round half to even, as rint
            free[y][x] = P; held[y][x] = r
            M[y][x] = r if src_mask is None else min(r, int(src_mask[y][x]))
    return held, M, free


def hold_case(h, w, K, seed, field="random", with_mask=True, unmasked=None):
    """inputs of the rule alone -> dict(pulled, label, prev, lab, lab_prev, field, src_mask). field: None, "zero", "random" (vectors up to +-3) or "extreme" (+-300:
    every vector is clamped); unmasked: the index of a reference without a mask (None: every reference has one). The maps hold 0, 255 and values between"""
    rng = np.random.default_rng(seed)

    def bytemap():
        m = rng.integers(0, 256, (h, w), dtype=np.uint8)
        m.reshape(-1)[::3] = 0; m.reshape(-1)[1::3] = 255
        return m
    pulled = [None if k == unmasked else bytemap() for k in range(K)]
    label = rng.integers(0, K, (h, w), dtype=np.uint8) if K > 1 else None
    prev = bytemap()[::-1].copy()
    lab = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    labp = np.clip(lab.astype(int) + rng.integers(-4, 5, (h, w, 3)), 0, 255).astype(np.uint8)
    labp[h // 3:h // 3 + max(1, h // 4), w // 3:w // 3 + max(1, w // 4)] = rng.integers(0, 256, 3, dtype=np.uint8)
    labp[:max(1, h // 5)] = lab[:max(1, h // 5)]               # rows that did not change: g = 1 with a zero field
    f = {None: None, "zero": np.zeros((h, w, 2), np.int16), "random": rng.integers(-3, 4, (h, w, 2)).astype(np.int16),
         "extreme": (300 * rng.choice([-1, 1], (h, w, 2))).astype(np.int16)}[field]
    return dict(pulled=pulled, label=label, prev=prev, lab=lab, lab_prev=labp, field=f, src_mask=bytemap() if with_mask else None)


def args_of(c):
    return c["pulled"], c["label"], c["prev"], c["lab"], c["lab_prev"], c["field"], c["src_mask"]


# ---- the composition

def _finish(orc, Xm, ah, aw, src, m, Pp, protect, form, full):
    """rules 6-8 on a mixed map: F at the working size, and with full = (S0, M0 or None, finish, sigma) the last level's F at the original size, which the exact finish
    and the masked upsampling finish compose with -> (working image, result, the F that the report names)"""
    H, W = src.shape[:2]
    F = refregion_ref.target_mask(orc, Pp, H, W, m)
    if full is None:
        work, out = seq_region_ref.finish(orc, Xm, ah, aw, src, F, protect, form, None)
        return work, out, F
    S0, M0, kind, sigma = full
    F0 = refregion_ref.target_mask(orc, Pp, *S0.shape[:2], M0)
    work, out = seq_region_ref.finish(orc, Xm, ah, aw, src, F, protect, form, (S0, F0, kind, sigma))
    return work, out, (F0 if kind == 0 else F)


def frame(orc, src, m, Rs, qs, ws, bs, state, tau, sigma, hold, mot=None, levels=5, protect=0, form=0, full=None, stale=False, hold_pull=True, seed=1, bds=2.0, iters=10):
    """one full frame: seq_multi_ref.frame's level loop with refregion_ref's pull behind each masked reference's votes, rule 3's hold, seq_region_ref's mix out of place and
    its finishes. m: the source mask at src's size or None; qs: per reference its mask at the reference's working size or None; state: None or the list per level of
    (X', L, labels, P'); stale: the kept P' belongs to other masks — the frame keeps P_l; hold_pull False: the free pull on every frame (the quality figure's baseline).
    -> (result, keep, new state); keep per level: seq_multi_ref.frame's maps, "pulled" [k][l], "p_free", "p_held", "mask", "mask_full", "ab_mix\""""
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    K = len(Rs)
    simg = multi_ref.pyramid(orc, src)
    mimg = region_ref.mask_pyramid(orc, m) if m is not None else [None] * 5
    qimg = [None if q is None else region_ref.mask_pyramid(orc, q) for q in qs]
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann, bnn = [None] * K, [None] * K
    keep = {k: [[] for _ in range(K)] for k in ("ref_err", "ref_guide", "pulled", "ref_mask")}
    keep.update({k: [] for k in ("free_label", "margin", "label", "guide", "err", "ab_nonlocal", "ab_blend", "tau_map", "motion", "result", "p_free", "p_held", "mask",
                                 "mask_full", "ab_mix")})
    new_state = []
    out = work = None
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    blends = tau > 0 and state is not None
    field = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        na = orc.feat_normalize(sfeat)
        guides, errs, pulled = [], [], []
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
            pulled.append(None if qimg[k] is None else refregion_ref.pull(qimg[k][l], ann[k], bnn[k], 1.0, bds))
            keep["ref_err"][k].append(errs[-1]); keep["ref_guide"][k].append(guides[-1]); keep["pulled"][k].append(pulled[-1])
            keep["ref_mask"][k].append(None if qimg[k] is None else qimg[k][l])
        L = orc.bgr2lab(simg[l])
        mo = np.zeros((ah, aw, 2), np.int16)
        if blends and on:
            mo = field = seq_mc_ref.motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
        if K == 1:
            lab = free = np.zeros((ah, aw), np.uint8); margin = np.zeros((ah, aw))
        elif blends and hold > 0:
            lab, free, margin = seq_multi_ref.select_hold(errs, state[l][2], L, state[l][1], mo if on else None, hold, sigma)
        else:
            lab = free = multi_ref.select(errs); margin = np.zeros((ah, aw))
        G, E = multi_ref.merge(lab, guides, errs)
        # rules 2-4
        if blends and hold_pull and not stale and state[l][3] is not None:
            Pp, M, P = pull_hold(pulled, lab if K > 1 else None, state[l][3], L, state[l][1], mo if on else None, mimg[l], tau, sigma)
        else:
            P = refregion_ref.merge(lab, pulled)
            Pp = P
            M = P if mimg[l] is None else np.minimum(P, mimg[l])
        knn_id, knn_w = orc.knn_graph(L, labels, nl, 1 << l)
        _, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        if blends:
            Xb, tp = seq_mc_ref.blend_mc(X, state[l][0], L, state[l][1], tau, sigma, mo if on else None)
        else:
            Xb, tp = X.copy(), np.zeros((ah, aw))
        new_state.append((Xb, L, lab, Pp))                     # the state is never mixed
        Xm = region_ref.mix(Xb, M)
        work, out, F = _finish(orc, Xm, ah, aw, src, m, Pp, protect, form, full if l == levels - 1 else None)
        for name, val in (("free_label", free), ("margin", margin), ("label", lab), ("guide", G), ("err", E), ("ab_nonlocal", X), ("ab_blend", Xb), ("tau_map", tp),
                          ("motion", mo), ("result", out), ("p_free", P), ("p_held", Pp), ("mask", M), ("mask_full", F), ("ab_mix", Xm)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(work, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state


def frame_propagate(orc, src, m, state, mot=None, levels=5, protect=0, form=0, full=None):
    """one propagated frame: seq_multi_ref.frame_propagate's warp of the unmixed state and carry of the labels, the kept P' carried the same way, then rules 4-8 on the
    last level run only -> (result, keep, new state); keep gains "p_held" per level and the last level run's "mask", "mask_full", "ab_mix\""""
    src = np.ascontiguousarray(src, np.uint8)
    _, keep, st = seq_multi_ref.frame_propagate(orc, src, state, mot=mot, levels=levels)
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    new_state = [(st[l][0], st[l][1], st[l][2], seq_multi_ref.carry(state[l][3], keep["motion"][l] if on else None)) for l in range(levels)]
    top = levels - 1
    Pp = new_state[top][3]
    ah, aw = Pp.shape
    mtop = None if m is None else region_ref.mask_pyramid(orc, m)[top]
    M = Pp if mtop is None else np.minimum(Pp, mtop)
    Xm = region_ref.mix(new_state[top][0], M)
    _, out, F = _finish(orc, Xm, ah, aw, src, m, Pp, protect, form, full)
    keep["p_held"] = [s[3] for s in new_state]
    keep["mask"], keep["mask_full"], keep["ab_mix"] = M, F, Xm
    return out, keep, new_state


def sequence(orc, frames, masks, refs, qs, ws, bs, kinds=KINDS, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, hold=seq_multi_ref.HOLD, mot=None, levels=5, protect=0, form=0,
             fulls=None, reset_before=(), hold_pull=True):
    """frames by their kinds ("F" / "B": a full frame; "P": propagated) under the source masks masks[t] (None: none; masks None: none on any frame) and the reference masks
    qs — a list of K masks / None in force on every frame, or a list per frame of such lists: a frame whose list is not the previous frame's finds the kept P' stale.
    fulls[t] = (S0, M0 or None, finish, sigma); reset_before: frames in front of which the sequence is reset -> (results, keeps, states)"""
    Rs = seq_multi_ref.prepare_references(orc, refs, ws, bs)
    per_frame = len(qs) == len(frames) and isinstance(qs[0], (list, tuple))
    state, outs, keeps, states = None, [], [], []
    last_q = None
    for t, (f, k) in enumerate(zip(frames, kinds)):
        if t in reset_before:
            state = None
        q = qs[t] if per_frame else qs
        stale = last_q is not None and any(a is not b for a, b in zip(q, last_q))
        m = None if masks is None else masks[t]
        full = None if fulls is None else fulls[t]
        if k == "P":
            assert not stale, "a propagated frame right after a mask change is refused (SPEC §6.19)"
            out, keep, state = frame_propagate(orc, f, m, state, mot=mot, levels=levels, protect=protect, form=form, full=full)
        else:
            out, keep, state = frame(orc, f, m, Rs, q, ws, bs, state, tau, sigma, hold, mot=mot, levels=levels, protect=protect, form=form, full=full, stale=stale,
                                     hold_pull=hold_pull)
        last_q = q
        outs.append(out); keeps.append(keep); states.append(state)
    return outs, keeps, states


def fullres_sequence(orc, frames0, masks0, refs0, qs0, ws, bs, max_side, finish_kind, guided_sigma=None, **kw):
    """a full-resolution sequence: frames, references and every mask shrunk by nct_working_size's rule (the masks by nct_resize_u8c1), the sequence at the working size,
    every frame's last finish on its original"""
    wh, ww = fullres_ref.working_size(*frames0[0].shape[:2], max_side)
    shrunk = (wh, ww) != tuple(frames0[0].shape[:2])
    S = [orc.resize_u8c3(np.ascontiguousarray(f, np.uint8), wh, ww) if shrunk else np.ascontiguousarray(f, np.uint8) for f in frames0]
    M = None if masks0 is None else [None if m is None else (region_ref.resize_u8c1(orc, m, wh, ww) if shrunk else np.ascontiguousarray(m, np.uint8)) for m in masks0]
    refs, qs = [], []
    for r0, q0 in zip(refs0, qs0):
        r0 = np.ascontiguousarray(r0, np.uint8)
        rh, rw = fullres_ref.working_size(*r0.shape[:2], max_side)
        small = (rh, rw) != tuple(r0.shape[:2])
        refs.append(orc.resize_u8c3(r0, rh, rw) if small else r0)
        qs.append(None if q0 is None else (region_ref.resize_u8c1(orc, q0, rh, rw) if small else np.ascontiguousarray(q0, np.uint8)))
    fulls = [(np.ascontiguousarray(f, np.uint8), None if masks0 is None or masks0[t] is None else np.ascontiguousarray(masks0[t], np.uint8), finish_kind, guided_sigma)
             for t, f in enumerate(frames0)]
    return sequence(orc, S, M, refs, qs, ws, bs, fulls=fulls, **kw)


# ---- the quality figure: how much the mask that drives the mix changes from frame to frame on a scene that does not

def pull_flicker(keeps, level=-1):
    """the mean |P'_t - P'_(t-1)| on a level run (default: the last one) over the frames after the first, in byte units"""
    d = [np.abs(keeps[t]["p_held"][level].astype(np.int64) - keeps[t - 1]["p_held"][level].astype(np.int64)).mean() for t in range(1, len(keeps))]
    return float(np.mean(d))
