"""Region tracking (SPEC §6.14): the carry of a matte along a motion field restated in numpy on int64, and the composition of a tracked sequence — the fields of
seq_mc_ref's search chained to the top level run, the matte carried frame by frame at the size frames arrive, and from there seq_region_ref's masked sequence fed the
carried mattes. No new reference arithmetic beside the rule: those modules are imported, not edited. Shared by tests/test_seq_track.py (CPU) and
tests/test_gpu_seq_track.py."""
import numpy as np

import fullres_ref
import multi_ref
import region_ref
import seq_mc_ref
import seq_region_ref


def axis(N, n):
    """rule 1 for one axis: the target coordinates 0 … N-1 on a grid of n -> (s, s1, t, D), int64 [N] and the denominator 2N of the fraction t / D"""
    x = np.arange(N, dtype=np.int64)
    D = 2 * N
    num = (2 * x + 1) * n - N
    s = num // D                                               # floor division
    t = num - s * D
    lo = s < 0
    s[lo] = 0; t[lo] = 0
    hi = s >= n - 1
    s[hi] = n - 1; t[hi] = 0
    return s, np.minimum(s + 1, n - 1), t, D


def displacement(field, H, W):
    """rule 1: field int16 [h][w][2] of (my, mx) -> (d_y, d_x) int64 [H][W], the vector in target pixels, rounded half up"""
    f = np.asarray(field, np.int16).astype(np.int64)
    h, w = f.shape[:2]
    assert 1 <= h <= H and 1 <= w <= W
    sy, sy1, ty, Dy = axis(H, h)
    sx, sx1, tx, Dx = axis(W, w)
    wy0, wy1 = (Dy - ty)[:, None], ty[:, None]
    wx0, wx1 = (Dx - tx)[None, :], tx[None, :]
    out = []
    for c, (N, n) in enumerate(((H, h), (W, w))):
        m = f[..., c]
        S = wy0 * wx0 * m[sy[:, None], sx[None, :]] + wy0 * wx1 * m[sy[:, None], sx1[None, :]] + wy1 * wx0 * m[sy1[:, None], sx[None, :]] + wy1 * wx1 * m[sy1[:, None], sx1[None, :]]
        den = n * Dy * Dx
        out.append((2 * S * N + den) // (2 * den))
    return out[0], out[1]


def matte_warp(mask, field):
    """nct_seq_matte_warp: mask [H][W] bytes, field int16 [h][w][2] -> mask read at the clamped p + d(p); a byte is copied"""
    m = np.ascontiguousarray(mask, np.uint8)
    H, W = m.shape
    dy, dx = displacement(field, H, W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.int64)
    return np.ascontiguousarray(m[np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)])


def labs(orc, frame, levels):
    """L_t[l] for the levels that run: what a frame leaves of itself in the state, and what the next frame's search reads"""
    simg = multi_ref.pyramid(orc, frame)
    return [orc.bgr2lab(simg[l]) for l in range(levels)]


def top_field(cur, prev, mot):
    """the field of the top level run of a frame against the previous one, from the two frames' labs(): seq_mc_ref.motion down the parent chain"""
    field = None
    for l, (L, Lp) in enumerate(zip(cur, prev)):
        field = seq_mc_ref.motion(L, Lp, field, mot[0] if l == 0 else mot[1], mot[2])
    return field


def carried(orc, frames, mattes, mot, levels, zero_at=(), tracking_from=0):
    """rule 2 over a clip of working-size frames: mattes[t] is the matte nct_seq_set_region gives before frame t (None: none given). A given matte is used as it came,
    age 0; else the previous matte is carried through the frame's top field — a zero field (it stays) for frame 0, with motion off (mot None or both radii 0) and for
    the frames in zero_at (after a reset, CUT frames) — and the age counts. -> (list of mattes at their own size, list of ages)"""
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    out, ages = [], []
    prev_labs, cur, age = None, None, 0
    for t, f in enumerate(frames):
        cur_labs = labs(orc, f, levels) if on else None
        if mattes[t] is not None:
            cur, age = np.ascontiguousarray(mattes[t], np.uint8), 0
        elif t >= tracking_from:
            assert cur is not None
            age += 1
            if on and t > 0 and t not in zero_at:
                cur = matte_warp(cur, top_field(cur_labs, prev_labs, mot))
        out.append(cur); ages.append(age)
        prev_labs = cur_labs
    return out, ages


def sequence(orc, frames, mattes, ref, ws, bs, mot=None, levels=5, **kw):
    """a tracked working-size sequence: seq_region_ref.sequence under the carried mattes -> (results, keeps, states, carried mattes, ages)"""
    M, ages = carried(orc, frames, mattes, mot, levels, zero_at=kw.get("reset_before", ()))
    outs, keeps, states = seq_region_ref.sequence(orc, frames, M, ref, ws, bs, mot=mot, levels=levels, **kw)
    return outs, keeps, states, M, ages


def fullres_sequence(orc, frames0, mattes0, ref0, ws, bs, max_side, finish_kind, guided_sigma=None, mot=None, levels=5, **kw):
    """a tracked full-resolution sequence: the fields come from the working-size frames, the matte is carried at the original size; seq_region_ref.fullres_sequence
    then shrinks each carried matte with nct_resize_u8c1, as nct_seq_set_region does -> (results, keeps, states, carried mattes, ages)"""
    wh, ww = fullres_ref.working_size(*frames0[0].shape[:2], max_side)
    shrunk = (wh, ww) != tuple(frames0[0].shape[:2])
    S = [orc.resize_u8c3(np.ascontiguousarray(f, np.uint8), wh, ww) if shrunk else np.ascontiguousarray(f, np.uint8) for f in frames0]
    M0, ages = carried(orc, S, mattes0, mot, levels)
    outs, keeps, states = seq_region_ref.fullres_sequence(orc, frames0, M0, ref0, ws, bs, max_side, finish_kind, guided_sigma, mot=mot, levels=levels, **kw)
    return outs, keeps, states, M0, ages


def rect(h, w, y0, y1, x0, x1):
    """a binary rectangle matte"""
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def shifted(m, dx):
    """the matte of a pan of dx px to the right per unit: what was at x + dx is now at x, the border clamped"""
    h, w = m.shape
    return np.ascontiguousarray(m[:, np.clip(np.arange(w) + dx, 0, w - 1)])


def iou(a, b):
    a, b = np.asarray(a) >= 128, np.asarray(b) >= 128
    u = (a | b).sum()
    return 1.0 if u == 0 else float((a & b).sum()) / float(u)


# field grid -> target of the seams: the smallest, one field vector for a whole target, equal sizes (d = m), ratio 4 twice (W % 4 == 0), a non-integer ratio with partial
# tiles, a ratio barely above 1 (the widest tap window), several tiles with W % 4 != 0
SEAM_CASES = [((1, 1), (1, 1)), ((1, 1), (8, 32)), ((9, 11), (9, 11)), ((9, 11), (36, 44)), ((14, 16), (56, 64)), ((17, 21), (45, 70)), ((33, 40), (34, 41)), ((5, 7), (67, 131))]
FIELD_KINDS = ("random", "zero", "constant", "extreme")


def seam_inputs(case, kind, seed=11):
    """-> (mask [H][W] random bytes, field int16 [h][w][2]): vectors in [-63, 63]; zeros; one constant vector; the int16 extremes and vectors that leave the grid"""
    (h, w), (H, W) = SEAM_CASES[case]
    rng = np.random.default_rng(seed + 100 * case)
    mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == "zero":
        field = np.zeros((h, w, 2), np.int16)
    elif kind == "constant":
        field = np.empty((h, w, 2), np.int16); field[..., 0] = 1; field[..., 1] = -2
    elif kind == "extreme":
        field = rng.integers(-3 * max(H, W) - 5, 3 * max(H, W) + 6, (h, w, 2)).astype(np.int16)
        flat = field.reshape(-1, 2)
        flat[::3] = rng.choice(np.array([-32767, 32767, 0], np.int16), (len(flat[::3]), 2))
    else:
        field = rng.integers(-63, 64, (h, w, 2)).astype(np.int16)
    return mask, field
