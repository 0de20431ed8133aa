"""Correspondence carry of frame sequences (SPEC §6.23): the moves of the kept fields (rules 3-4) and the merge (rule 6) restated in numpy, and seq_mc_ref's composition
with rules 2-6 in front of every level's PatchMatch and propagated frames in between. Shared by tests/test_seq_carry.py (CPU) and tests/test_gpu_seq_carry.py.
Everything in the moves is integer arithmetic; the merge compares the oracle's step-0 distances (patchmatch(..., iters=0)) as fp32."""
import numpy as np

import fullres_ref
import multi_ref
import seq_mc_ref
import seq_prop_ref
import seq_ref

HOLE = np.uint32(0xFFFFFFFF)


def word(y, x):
    return (np.asarray(y, np.int64) << 12 | np.asarray(x, np.int64)).astype(np.uint32)


def _target(field):
    """the clamped p + m(p) of every p -> (ty, tx) int64 [h][w]"""
    f = np.asarray(field, np.int16).astype(np.int64)
    h, w = f.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    return np.clip(yy + f[..., 0], 0, h - 1), np.clip(xx + f[..., 1], 0, w - 1)


def move_a(a, field):
    """rule 3: A'(p) = A(p + m(p)), the 32-bit word copied through the component-wise clamped vector"""
    ty, tx = _target(field)
    return np.ascontiguousarray(np.asarray(a, np.uint32).reshape(ty.shape)[ty, tx])


def forward_map(field):
    """rule 4: F(s) = min { word(p) : p + m(p) = s }, and word(clamp(s - m(s))) where no p lands on s -> uint32 [h][w]"""
    f = np.asarray(field, np.int16).astype(np.int64)
    h, w = f.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    ty, tx = _target(field)
    F = np.full(h * w, HOLE, np.uint32)
    np.minimum.at(F, (ty * w + tx).reshape(-1), word(yy, xx).reshape(-1))
    F = F.reshape(h, w)
    back = word(np.clip(yy - f[..., 0], 0, h - 1), np.clip(xx - f[..., 1], 0, w - 1))
    return np.where(F == HOLE, back, F)


def remap_b(b, fwd):
    """rule 4: B'(q) = F(B(q)); the word's coordinates are clamped to F's grid"""
    fwd = np.asarray(fwd, np.uint32)
    h, w = fwd.shape
    b = np.asarray(b, np.uint32)
    return np.ascontiguousarray(fwd[np.minimum((b >> 12) & 0xFFF, h - 1), np.minimum(b & 0xFFF, w - 1)])


def merge(dist, z, c):
    """rule 6: dist(field) -> fp32 step-0 distances; start = c where d_c < d_z strictly (a NaN keeps z) -> (start, d_z, d_c)"""
    z, c = np.asarray(z, np.uint32), np.asarray(c, np.uint32)
    dz, dc = np.asarray(dist(z), np.float32), np.asarray(dist(c), np.float32)
    with np.errstate(invalid="ignore"):
        take = dc < dz
    return np.where(take, c, z).astype(np.uint32), dz, dc


# ---- scalar python loops of the same rules, for the CPU test of the numpy forms

def loop_move_a(a, field):
    h, w = field.shape[:2]
    out = np.zeros((h, w), np.uint32)
    for y in range(h):
        for x in range(w):
            out[y, x] = a[min(max(y + int(field[y, x, 0]), 0), h - 1), min(max(x + int(field[y, x, 1]), 0), w - 1)]
    return out


def loop_forward_map(field):
    h, w = field.shape[:2]
    F = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            ty, tx = min(max(y + int(field[y, x, 0]), 0), h - 1), min(max(x + int(field[y, x, 1]), 0), w - 1)
            v = (y << 12) | x
            F[ty][tx] = v if F[ty][tx] is None else min(F[ty][tx], v)
    holes = 0
    for y in range(h):
        for x in range(w):
            if F[y][x] is None:
                holes += 1
                F[y][x] = (min(max(y - int(field[y, x, 0]), 0), h - 1) << 12) | min(max(x - int(field[y, x, 1]), 0), w - 1)
    return np.array(F, np.uint32), holes


def loop_remap_b(b, fwd):
    h, w = fwd.shape
    out = np.zeros(b.shape, np.uint32)
    for y in range(b.shape[0]):
        for x in range(b.shape[1]):
            v = int(b[y, x])
            out[y, x] = fwd[min((v >> 12) & 0xFFF, h - 1), min(v & 0xFFF, w - 1)]
    return out


# ---- inputs of the seams

GRIDS = [((2, 2), (2, 3)), ((3, 7), (8, 5)), ((9, 33), (31, 40)), ((33, 70), (8, 5))]          # (source grid, reference grid)


def field_case(h, w, seed, kind):
    """int16 [h][w][2]. "random": vectors in +-3 (on small grids many leave it; several p land on one s and holes open); "outside": far outside, the int16 extremes
    among them; "shift": one vector everywhere (every s but a border strip is hit once); "zero" """
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((h, w, 2), np.int16)
    if kind == "shift":
        return np.broadcast_to(np.array([1, -2], np.int16), (h, w, 2)).copy()
    if kind == "outside":
        f = rng.integers(-3 * max(h, w) - 5, 3 * max(h, w) + 6, (h, w, 2)).astype(np.int16)
        f.reshape(-1, 2)[::3] = rng.choice(np.array([-32768, 32767, 0], np.int16), (len(f.reshape(-1, 2)[::3]), 2))
        return f
    return rng.integers(-3, 4, (h, w, 2)).astype(np.int16)


def nnf_case(h, w, th, tw, seed):
    """a field [h][w] of words into a grid th x tw"""
    rng = np.random.default_rng(seed)
    return word(rng.integers(0, th, (h, w)), rng.integers(0, tw, (h, w)))


# ---- the composition

def frame(orc, src, R, ws, bs, state, carry, tau, sigma, mot=None, levels=5, seed=1, bds=2.0, iters=10, carry_iters=None):
    """seq_mc_ref.frame of a carrying sequence. carry: None (the sequence holds no kept fields: a first frame, a frame after a reset) or the list per level of (A, B);
    carry_iters: PatchMatch iterations of a frame that merged (None: iters). -> (result, keep, new state, new carry); keep gains per level "start_a", "start_b", "ann",
    "bnn", "annd", "bnnd", and "dz_a", "dc_a" (None on a frame that did not merge)"""
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    simg = multi_ref.pyramid(orc, src)
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann = bnn = None
    keep = {k: [] for k in ("result", "ab_nonlocal", "ab_blend", "tau_map", "motion", "start_a", "start_b", "ann", "bnn", "annd", "bnnd", "dz_a", "dc_a")}
    new_state, new_carry = [], []
    out = None
    maxLen = max(H, W, *R["img"].shape[:2])
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    merged = carry is not None and state is not None
    it = iters if (not merged or carry_iters is None) else carry_iters
    field = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        bh, bw = R["pyr"][l].shape[:2]
        rs = [maxLen // 16, maxLen // 32, maxLen // 64, 32, 32][l]
        rf = R["taps"][4 - l]
        na, nb = orc.feat_normalize(sfeat), orc.feat_normalize(rf)
        L = orc.bgr2lab(simg[l])
        blend = tau > 0 and state is not None
        m = np.zeros((ah, aw, 2), np.int16)
        if on and (merged or blend):                               # rule 2: found once, in front of the correspondence
            m = field = seq_mc_ref.motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
        if l == 0:
            a0, b0 = orc.nnf_init(ah, aw, bh, bw), orc.nnf_init(bh, bw, ah, aw)
        else:
            a0, b0 = orc.nnf_upsample(ann, ah, aw, bh, bw), orc.nnf_upsample(bnn, bh, bw, ah, aw)
        sab = (seed ^ (0x9E3779B9 * (2 * l + 1))) & 0xffffffff
        sba = (seed ^ (0x9E3779B9 * (2 * l + 2))) & 0xffffffff
        dz_a = dc_a = None
        if merged:
            ca, cb = carry[l]
            if on:
                ca, cb = move_a(ca, m), remap_b(cb, forward_map(m))
            a0, dz_a, dc_a = merge(lambda f: orc.patchmatch(na, nb, f, 0, rs, sab)[1], a0, ca)
            b0, _, _ = merge(lambda f: orc.patchmatch(nb, na, f, 0, rs, sba)[1], b0, cb)
        ann, annd = orc.patchmatch(na, nb, a0, it, rs, sab)
        bnn, bnnd = orc.patchmatch(nb, na, b0, it, rs, sba)
        new_carry.append((ann.copy(), bnn.copy()))
        G = orc.bds_vote_image(simg[l], R["pyr"][l], ann, bnn, 1.0, bds)
        E = orc.feature_distance(na, orc.feat_normalize(orc.bds_vote_features(ann, bnn, rf, 1.0, bds)))
        knn_id, knn_w = orc.knn_graph(L, labels, nl, 1 << l)
        out, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        if blend:
            if on:
                Xb, tp = seq_mc_ref.blend_mc(X, state[l][0], L, state[l][1], tau, sigma, m)
            else:
                Xb, tp = seq_ref.blend(X, state[l][0], L, state[l][1], tau, sigma)
            out, _ = fullres_ref.oracle_finish(orc, Xb, ah, aw, H, W, src)
        else:
            Xb, tp = X.copy(), np.zeros((ah, aw))
        new_state.append((Xb, L))
        for name, val in (("result", out), ("ab_nonlocal", X), ("ab_blend", Xb), ("tau_map", tp), ("motion", m), ("start_a", a0), ("start_b", b0), ("ann", ann), ("bnn", bnn),
                          ("annd", annd), ("bnnd", bnnd), ("dz_a", dz_a), ("dc_a", dc_a)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state, new_carry


def frame_multi(orc, src, Rs, ws, bs, state, carry, tau, sigma, hold, mot=None, levels=5, seed=1, bds=2.0, iters=10, carry_iters=None):
    """seq_multi_ref.frame of a carrying sequence over the references Rs: the kept fields are per reference (carry: None or [l][k] of (A, B)) and the level's field is
    found once, in front of the first reference's correspondence. -> (result, keep, new state, new carry); keep gains "ann", "bnn", "annd", "bnnd" as [k][l]"""
    import seq_multi_ref
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    K = len(Rs)
    simg = multi_ref.pyramid(orc, src)
    sfeat = orc.vgg19_features(src, ws, bs)[4]
    labels, nl = orc.cluster_features(sfeat, 10, 11, seed)
    ann, bnn = [None] * K, [None] * K
    keep = {k: [[] for _ in range(K)] for k in ("ann", "bnn", "annd", "bnnd")}
    keep.update({k: [] for k in ("label", "ab_blend", "motion", "result")})
    new_state, new_carry = [], []
    out = None
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    blends = tau > 0 and state is not None
    merged = carry is not None and state is not None
    it = iters if (not merged or carry_iters is None) else carry_iters
    field = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        na = orc.feat_normalize(sfeat)
        L = orc.bgr2lab(simg[l])
        m = np.zeros((ah, aw, 2), np.int16)
        if on and (merged or blends):
            m = field = seq_mc_ref.motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
        guides, errs = [], []
        new_carry.append([])
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
            if merged:
                ca, cb = carry[l][k]
                if on:
                    ca, cb = move_a(ca, m), remap_b(cb, forward_map(m))
                a0, _, _ = merge(lambda f: orc.patchmatch(na, nb, f, 0, rs, sab)[1], a0, ca)
                b0, _, _ = merge(lambda f: orc.patchmatch(nb, na, f, 0, rs, sba)[1], b0, cb)
            ann[k], annd = orc.patchmatch(na, nb, a0, it, rs, sab)
            bnn[k], bnnd = orc.patchmatch(nb, na, b0, it, rs, sba)
            new_carry[l].append((ann[k].copy(), bnn[k].copy()))
            for name, val in (("ann", ann[k]), ("bnn", bnn[k]), ("annd", annd), ("bnnd", bnnd)):
                keep[name][k].append(val)
            guides.append(orc.bds_vote_image(simg[l], R["pyr"][l], ann[k], bnn[k], 1.0, bds))
            errs.append(orc.feature_distance(na, orc.feat_normalize(orc.bds_vote_features(ann[k], bnn[k], rf, 1.0, bds))))
        if K == 1:
            lab = np.zeros((ah, aw), np.uint8)
        elif blends and hold > 0:
            lab, _, _ = seq_multi_ref.select_hold(errs, state[l][2], L, state[l][1], m if on else None, hold, sigma)
        else:
            lab = multi_ref.select(errs)
        G, E = multi_ref.merge(lab, guides, errs)
        knn_id, knn_w = orc.knn_graph(L, labels, nl, 1 << l)
        out, st = orc.local_color_transfer(E, simg[l], G, src, knn_id, knn_w, l, want_stages=True)
        X = st["ab_nonlocal"].reshape(2, ah * aw, 3)
        if blends:
            Xb, _ = seq_mc_ref.blend_mc(X, state[l][0], L, state[l][1], tau, sigma, m if on else None)
            out, _ = fullres_ref.oracle_finish(orc, Xb, ah, aw, H, W, src)
        else:
            Xb = X.copy()
        new_state.append((Xb, L, lab))
        for name, val in (("label", lab), ("ab_blend", Xb), ("motion", m), ("result", out)):
            keep[name].append(val)
        if l < levels - 1:
            sfeat = orc.vgg19_features(out, ws, bs, deepest_tap=4 - l)[4 - l - 1]
    return out, keep, new_state, new_carry


def sequence_multi(orc, frames, refs, ws, bs, carry_iters=None, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, hold=0.005, mot=None, levels=5):
    """full frames of a carrying sequence over several references -> (list of results, list of keeps, list of the kept fields [l][k] after each frame)"""
    Rs = [seq_ref.prepare_reference(orc, r, ws, bs) for r in refs]
    state = kept = None
    outs, keeps, carries = [], [], []
    for f in frames:
        out, keep, state, kept = frame_multi(orc, f, Rs, ws, bs, state, kept, tau, sigma, hold, mot=mot, levels=levels, carry_iters=carry_iters)
        outs.append(out); keeps.append(keep); carries.append(kept)
    return outs, keeps, carries


def propagate(orc, src, state, carry, mot=None, levels=5):
    """seq_prop_ref.frame_propagate, and rule 5: the kept fields follow every level's field -> (result, keep, new state, new carry)"""
    out, keep, new_state = seq_prop_ref.frame_propagate(orc, src, state, mot=mot, levels=levels)
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    if carry is not None and on:
        carry = [(move_a(a, m), remap_b(b, forward_map(m))) for (a, b), m in zip(carry, keep["motion"])]
    return out, keep, new_state, carry


def first_frame(orc, frame0, ref, ws, bs, levels=5, **kw):
    """the first frame of a sequence: it has no state and no kept fields, so it depends on neither tau, the motion settings nor carry_iters, and callers that run
    several sequences on the same frames may compute it once and hand it to sequence(first=...)"""
    R = seq_ref.prepare_reference(orc, ref, ws, bs)
    return frame(orc, frame0, R, ws, bs, None, None, seq_ref.TAU, seq_ref.SIGMA, levels=levels, **kw)


def sequence(orc, frames, ref, ws, bs, carry=True, carry_iters=None, plan=None, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, mot=None, levels=5, first=None, **kw):
    """a sequence with the carry on (or off: seq_mc_ref.sequence with the same reports); plan: per frame True = full, False = propagated (None: all full);
    first: first_frame's tuple for frames[0] -> (list of results, list of keeps, list of the kept fields after each frame)"""
    R = seq_ref.prepare_reference(orc, ref, ws, bs)
    state = kept = None
    outs, keeps, carries = [], [], []
    for t, (f, whole) in enumerate(zip(frames, plan or [True] * len(frames))):
        if t == 0 and first is not None:
            out, keep, state, kept = first
        elif whole:
            out, keep, state, new = frame(orc, f, R, ws, bs, state, kept if carry else None, tau, sigma, mot=mot, levels=levels, carry_iters=carry_iters, **kw)
            kept = new
        else:
            out, keep, state, kept = propagate(orc, f, state, kept, mot=mot, levels=levels)
        outs.append(out); keeps.append(keep); carries.append(kept)
    return outs, keeps, carries
