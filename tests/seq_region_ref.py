"""Region masks in sequences (SPEC §6.13) composed from the oracle's exported stages: the level loop of seq_mc_ref.frame (seq_ref.frame's, with §6.4's field where motion
is on) with region_ref's mix and compose inserted as §6.13 orders them, the propagated frame on top of seq_prop_ref, the exact finish on top of fullres_ref, and the masked
upsampling finish as the chain finish_up_ref / finish_guided_ref -> region_ref.keep_map -> compose. No new reference arithmetic: those modules are imported, not edited.
Shared by tests/test_seq_region.py (CPU) and tests/test_gpu_seq_region.py. The state a frame returns is never mixed: it is the unmasked sequence's wherever the
features a level sees are the unmasked sequence's (always at level 0)."""
import numpy as np

import finish_guided_ref
import finish_up_ref
import fullres_ref
import multi_ref
import region_ref
import seq_mc_ref
import seq_prop_ref
import seq_ref

KINDS = "FBPB"                   # the frame kinds of the tests' plan: full (first), blended, propagated, blended


def masked_finish(orc, ab_wls, h, w, s_bgr_full, m0, protect=0, form=None, lab_w=None, sigma=None):
    """§6.13 rule 4, the masked upsampling finish: Lab_o from the upsampling finish (lab_w None) or the guided one (lab_w: the working-size guide, sigma), then per
    original pixel out = keep ? S0 : Lab2BGR(Lab_o) -> (bgr, lab_o)"""
    s = np.ascontiguousarray(s_bgr_full, np.uint8)
    if lab_w is None:
        bgr, olab = finish_up_ref.oracle_finish_upsample(orc, ab_wls, h, w, s, form)
    else:
        bgr, olab = finish_guided_ref.finish_guided(orc, ab_wls, lab_w, h, w, s, finish_guided_ref.SIGMA if sigma is None else sigma, form)
    keep = region_ref.keep_map(orc.bgr2lab(s), olab, m0, protect)
    return np.where(keep[..., None], s, bgr), olab


def finish(orc, xm, ah, aw, src, m, protect=0, form=0, full=None):
    """rule 4 on a mixed map xm of the level grid ah x aw: the working-size finish and compose, or with full = (S0, M0, finish, sigma) the exact finish and compose on
    the original (finish 0) / the working-size finish and the masked upsampling finish behind it (finish 1; sigma None: plain, else guided)
    -> (the working-size image the next level's re-predict reads, the frame's result)"""
    H, W = src.shape[:2]
    if full is not None and full[2] == 0:
        S0, M0 = full[0], full[1]
        _, fin = fullres_ref.oracle_finish(orc, xm, ah, aw, H, W, S0, form)
        return None, region_ref.compose(orc, S0, fin["lab"], M0, protect, form)
    _, fin = fullres_ref.oracle_finish(orc, xm, ah, aw, H, W, src, form)
    work = region_ref.compose(orc, src, fin["lab"], m, protect, form)
    if full is None:
        return work, work
    S0, M0, _, sigma = full
    out0, _ = masked_finish(orc, fin["ab_wls"], H, W, S0, M0, protect, form, None if sigma is None else orc.bgr2lab(src), sigma)
    return work, out0


def frame(orc, src, m, R, ws, bs, state, tau, sigma, mot=None, levels=5, protect=0, form=0, full=None, seed=1, bds=2.0, iters=10):
    """one full frame (rule 2): per level S1, the blend into the state, the mix out of place, the finish on the mixed map, the compose. m: the mask at src's size.
    -> (result, keep, new state); keep: per level "result", "ab_nonlocal", "ab_blend" (the unmixed X'_t), "ab_mix", "mask", "tau_map", "motion" """
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    simg = multi_ref.pyramid(orc, src)
    mimg = region_ref.mask_pyramid(orc, m)
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann = bnn = None
    keep = {k: [] for k in ("result", "ab_nonlocal", "ab_blend", "ab_mix", "mask", "tau_map", "motion")}
    new_state = []
    out = work = None
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
        _, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        mo = np.zeros((ah, aw, 2), np.int16)
        if tau > 0 and state is not None:
            if on:
                mo = field = seq_mc_ref.motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
                Xb, tp = seq_mc_ref.blend_mc(X, state[l][0], L, state[l][1], tau, sigma, mo)
            else:
                Xb, tp = seq_ref.blend(X, state[l][0], L, state[l][1], tau, sigma)
        else:
            Xb, tp = X.copy(), np.zeros((ah, aw))
        new_state.append((Xb, L))                              # the state is never mixed
        Xm = region_ref.mix(Xb, mimg[l])
        work, out = finish(orc, Xm, ah, aw, src, m, protect, form, full if l == levels - 1 else None)
        for name, val in (("result", out), ("ab_nonlocal", X), ("ab_blend", Xb), ("ab_mix", Xm), ("mask", mimg[l]), ("tau_map", tp), ("motion", mo)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(work, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state


def frame_propagate(orc, src, m, state, mot=None, levels=5, protect=0, form=0, full=None):
    """one propagated frame (rule 3): seq_prop_ref.frame_propagate's warp of the unmixed state, then the last level run's X'_t mixed with that level's mask, the finish on
    the mixed map and the compose -> (result, keep, new state); keep gains "ab_mix" and "mask" (the last level run's only)"""
    src = np.ascontiguousarray(src, np.uint8)
    _, keep, new_state = seq_prop_ref.frame_propagate(orc, src, state, mot=mot, levels=levels)
    top = levels - 1
    mtop = region_ref.mask_pyramid(orc, m)[top]
    ah, aw = mtop.shape
    Xm = region_ref.mix(new_state[top][0], mtop)
    _, out = finish(orc, Xm, ah, aw, src, m, protect, form, full)
    keep["ab_mix"], keep["mask"] = Xm, mtop
    return out, keep, new_state


def sequence(orc, frames, masks, ref, ws, bs, kinds=KINDS, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, mot=None, levels=5, protect=0, form=0, fulls=None, reset_before=()):
    """frames by their kinds ("F" / "B": a full frame — blended where there is state; "P": propagated), frame t under masks[t] (None: the unmasked frame of
    seq_mc_ref / seq_prop_ref); fulls[t] = (S0, M0, finish, sigma) for a full-resolution sequence; reset_before: frames in front of which the sequence is reset
    -> (results, keeps, states)"""
    R = seq_ref.prepare_reference(orc, ref, ws, bs)
    state, outs, keeps, states = None, [], [], []
    for t, (f, k) in enumerate(zip(frames, kinds)):
        if t in reset_before:
            state = None
        full = None if fulls is None else fulls[t]
        if masks[t] is None:
            assert full is None
            if k == "P":
                out, keep, state = seq_prop_ref.frame_propagate(orc, f, state, mot=mot, levels=levels)
            else:
                out, keep, state = seq_mc_ref.frame(orc, f, R, ws, bs, state, tau, sigma, mot=mot, levels=levels)
        elif k == "P":
            out, keep, state = frame_propagate(orc, f, masks[t], state, mot=mot, levels=levels, protect=protect, form=form, full=full)
        else:
            out, keep, state = frame(orc, f, masks[t], R, ws, bs, state, tau, sigma, mot=mot, levels=levels, protect=protect, form=form, full=full)
        outs.append(out); keeps.append(keep); states.append(state)
    return outs, keeps, states


def fullres_sequence(orc, frames0, masks0, ref0, ws, bs, max_side, finish_kind, guided_sigma=None, **kw):
    """a full-resolution sequence (§6.9 with rule 4): frames, masks and the reference shrunk by nct_working_size's rule (the mask by nct_resize_u8c1), the sequence at
    the working size, every frame's last finish on its original with the mask at the original size"""
    wh, ww = fullres_ref.working_size(*frames0[0].shape[:2], max_side)
    rh, rw = fullres_ref.working_size(*ref0.shape[:2], max_side)
    shrunk = (wh, ww) != tuple(frames0[0].shape[:2])
    S = [orc.resize_u8c3(np.ascontiguousarray(f, np.uint8), wh, ww) if shrunk else np.ascontiguousarray(f, np.uint8) for f in frames0]
    M = [region_ref.resize_u8c1(orc, m, wh, ww) if shrunk else np.ascontiguousarray(m, np.uint8) for m in masks0]
    ref = orc.resize_u8c3(np.ascontiguousarray(ref0, np.uint8), rh, rw) if (rh, rw) != tuple(ref0.shape[:2]) else ref0
    fulls = [(np.ascontiguousarray(f, np.uint8), np.ascontiguousarray(m, np.uint8), finish_kind, guided_sigma) for f, m in zip(frames0, masks0)]
    return sequence(orc, S, M, ref, ws, bs, fulls=fulls, **kw)


# ---- inputs of the masked finish seams: (working grid h x w) -> (target H x W): ratio 4; a non-integer ratio with partial tiles on both axes; a ratio barely above 1 (the
# widest tap window); the smallest grid; equal sizes (the copy path)
SEAM_CASES = [((14, 16), (56, 64)), ((43, 64), (90, 131)), ((32, 40), (33, 41)), ((1, 1), (8, 32)), ((17, 19), (17, 19))]


def seam_inputs(orc, case):
    """-> (ab_wls, lab_w, h, w, s_full, mask): smooth coefficients that are exactly (a, b) = (1, +0.0) on a band of working pixels — there Lab does not move, whatever the
    stretch — and a mask with 0, 255 and partial values both inside and outside that band, so that every outcome of the compose occurs"""
    import synth
    (h, w), (H, W) = SEAM_CASES[case]
    ab = fullres_ref.smooth_ab(700 + case, h, w).reshape(2, h, w, 3).copy()
    s_full = synth.image(800 + case, H, W)
    lab_w = orc.bgr2lab(orc.resize_u8c3(s_full, h, w)) if (h, w) != (H, W) else orc.bgr2lab(s_full)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = ((xx * 7 + yy * 13) % 256).astype(np.uint8)          # every byte value where the target has room
    mask[(yy % 4 == 0)] = 0
    mask[(yy % 4 == 1)] = 255
    if h > 1:
        ab[0, : (h + 1) // 2] = 1.0; ab[1, : (h + 1) // 2] = 0.0
    else:                                                      # one working pixel: the identity everywhere; "converted" then comes from M == 255 rows, kept from the others
        ab[0] = 1.0; ab[1] = 0.0
    return ab.reshape(2, h * w, 3), lab_w, h, w, s_full, mask


def outcome_shares(orc, lab_o, s_full, mask, protect):
    """the share of pixels kept by protect (M == 0), kept because Lab did not move under 0 < M < 255, and converted"""
    lab_s = orc.bgr2lab(np.ascontiguousarray(s_full, np.uint8))
    m = np.asarray(mask, np.uint8)
    keep = region_ref.keep_map(lab_s, lab_o, m, protect)
    same = (np.asarray(lab_o) == lab_s).all(axis=-1)
    return float((keep & (m == 0)).mean()), float((keep & same & (m != 0) & (m != 255)).mean()), float((~keep).mean())
