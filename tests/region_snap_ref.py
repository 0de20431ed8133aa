"""Matte snapping (SPEC §6.15): the rule restated in numpy on int64, and the composition of a tracked and snapped sequence — seq_track_ref's carry through the fields
of seq_mc_ref's search, the snap behind it with the frame's Lab image as the guide, and from there seq_region_ref's masked sequence fed those mattes. No new reference
arithmetic beside the rule: those modules are imported, not edited. Shared by tests/test_region_snap.py (CPU) and tests/test_gpu_region_snap.py."""
import numpy as np

import fullres_ref
import seq_ref
import seq_region_ref
import seq_track_ref as tr
import synth

RADIUS, SIGMA, BINARY = 3, 10, 1           # nct_region_snap_params_default


def snap(mask, lab, r=RADIUS, sigma=SIGMA, binary=BINARY):
    """nct_region_snap: mask [H][W] bytes, lab [H][W][3] bytes -> per pixel the mean of the matte over the taps of its (2r + 1)^2 window inside the image, weighted with
    max(0, 3 sigma^2 - d2) and rounded half up; binary: cut at 128"""
    M, L = np.asarray(mask, np.uint8).astype(np.int64), np.asarray(lab, np.uint8).astype(np.int64)
    H, W = M.shape
    assert L.shape == (H, W, 3) and 1 <= r <= 8 and 1 <= sigma <= 255 and binary in (0, 1)
    A, B = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if abs(dy) >= H or abs(dx) >= W:
                continue                                        # no pixel has this tap inside the image
            p = (slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx)))
            q = (slice(p[0].start + dy, p[0].stop + dy), slice(p[1].start + dx, p[1].stop + dx))
            w = np.maximum(0, 3 * sigma * sigma - ((L[p] - L[q]) ** 2).sum(axis=-1))
            A[p] += w * M[q]
            B[p] += w
    assert (B > 0).all()
    v = (2 * A + B) // (2 * B)
    return (np.where(v >= 128, 255, 0) if binary else v).astype(np.uint8)


def window_extremes(mask, r):
    """per pixel the least and the largest byte of the matte over its window inside the image"""
    m = np.asarray(mask, np.uint8)
    H, W = m.shape
    lo, hi = m.copy(), m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if abs(dy) >= H or abs(dx) >= W:
                continue
            p = (slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx)))
            q = (slice(p[0].start + dy, p[0].stop + dy), slice(p[1].start + dx, p[1].stop + dx))
            lo[p] = np.minimum(lo[p], m[q]); hi[p] = np.maximum(hi[p], m[q])
    return lo, hi


def carried_snapped(orc, frames, mattes, mot, levels, snap_params, zero_at=(), tracking_from=0, guides=None):
    """seq_track_ref.carried with the snap behind the carry (SPEC §6.15 rule 3). frames: at the working size, where the fields are found; guides: the frames at the size
    frames arrive (None: the same), whose Lab images guide the snap; snap_params: (r, sigma, binary), or None for the carry alone. A frame snaps where its age counts
    and the sequence has state: not frame 0, not the frames in zero_at (after a reset, CUT frames), with motion on or off -> (mattes at their own size, ages)"""
    if snap_params is None:
        return tr.carried(orc, frames, mattes, mot, levels, zero_at=zero_at, tracking_from=tracking_from)
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    guides = frames if guides is None else guides
    out, ages = [], []
    prev_labs, cur, age = None, None, 0
    for t, f in enumerate(frames):
        cur_labs = tr.labs(orc, f, levels) if on else None
        if mattes[t] is not None:
            cur, age = np.ascontiguousarray(mattes[t], np.uint8), 0
        elif t >= tracking_from:
            assert cur is not None
            age += 1
            if t > 0 and t not in zero_at:
                if on:
                    cur = tr.matte_warp(cur, tr.top_field(cur_labs, prev_labs, mot))
                cur = snap(cur, orc.bgr2lab(np.ascontiguousarray(guides[t], np.uint8)), *snap_params)
        out.append(cur); ages.append(age)
        prev_labs = cur_labs
    return out, ages


def sequence(orc, frames, mattes, ref, ws, bs, snap_params, mot=None, levels=5, **kw):
    """a tracked and snapped working-size sequence: seq_region_ref.sequence under the snapped mattes -> (results, keeps, states, mattes, ages)"""
    M, ages = carried_snapped(orc, frames, mattes, mot, levels, snap_params, zero_at=kw.get("reset_before", ()))
    outs, keeps, states = seq_region_ref.sequence(orc, frames, M, ref, ws, bs, mot=mot, levels=levels, **kw)
    return outs, keeps, states, M, ages


def fullres_sequence(orc, frames0, mattes0, ref0, ws, bs, max_side, finish_kind, snap_params, guided_sigma=None, mot=None, levels=5, **kw):
    """a tracked and snapped full-resolution sequence: the fields come from the working-size frames, the matte is carried and snapped at the original size with the
    original frame as the guide; seq_region_ref.fullres_sequence then shrinks each matte -> (results, keeps, states, mattes, ages)"""
    wh, ww = fullres_ref.working_size(*frames0[0].shape[:2], max_side)
    shrunk = (wh, ww) != tuple(frames0[0].shape[:2])
    S = [orc.resize_u8c3(np.ascontiguousarray(f, np.uint8), wh, ww) if shrunk else np.ascontiguousarray(f, np.uint8) for f in frames0]
    M0, ages = carried_snapped(orc, S, mattes0, mot, levels, snap_params, guides=frames0)
    outs, keeps, states = seq_region_ref.fullres_sequence(orc, frames0, M0, ref0, ws, bs, max_side, finish_kind, guided_sigma, mot=mot, levels=levels, **kw)
    return outs, keeps, states, M0, ages


OBJ_ROWS, OBJ_COLS, OBJ_BGR = (16, 40), (10, 38), (40, 60, 200)


def obj_frames(n, H, W, step):
    """the object clip: a 24 x 28 rectangle of one colour that moves `step` px per frame to the right over a still synth image, under fresh noise per frame
    -> (frames, truth mattes: the rectangle of each frame)"""
    rng = np.random.default_rng(5)
    base = synth.image(1000, H, W)
    frames, truth = [], []
    for t in range(n):
        img = base.copy()
        x0, x1 = OBJ_COLS[0] + step * t, OBJ_COLS[1] + step * t
        assert x1 <= W and OBJ_ROWS[1] <= H
        img[OBJ_ROWS[0]:OBJ_ROWS[1], x0:x1] = OBJ_BGR
        frames.append(seq_ref._noisy(img, rng, 2.0))
        truth.append(tr.rect(H, W, OBJ_ROWS[0], OBJ_ROWS[1], x0, x1))
    return frames, truth


# the seams' targets: the smallest, a single row narrower than the r = 3 window, exactly one tile (W % 4 == 0), smaller than the r = 8 window with W % 4 != 0, several tiles with
# W % 4 != 0 and partial tiles, partial tiles both ways, many tiles with odd sides; crossed with every radius, sigma, binary, matte and guide kind below
SEAM_CASES = [(1, 1), (1, 7), (8, 32), (9, 11), (45, 70), (34, 41), (67, 131)]
RADII, SIGMAS, BINARIES = (1, 3, 8), (1, 10, 255), (0, 1)
MATTE_KINDS = ("random", "binary", "zero", "full")
GUIDE_KINDS = ("random", "flat", "regions")


def seam_inputs(case, matte_kind, guide_kind, seed=23):
    """-> (mask [H][W], lab [H][W][3]). Mattes: random bytes; random 0 / 255; all 0; all 255. Guides: random bytes (neighbours far apart: only a large sigma mixes); one
    colour (the box mean); two regions split down a diagonal, each its colour plus noise of a few units (weights between 0 and the largest)"""
    H, W = SEAM_CASES[case]
    rng = np.random.default_rng(seed + 100 * case)
    mask = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if matte_kind == "binary":
        mask = np.where(mask >= 128, 255, 0).astype(np.uint8)
    elif matte_kind == "zero":
        mask = np.zeros((H, W), np.uint8)
    elif matte_kind == "full":
        mask = np.full((H, W), 255, np.uint8)
    lab = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if guide_kind == "flat":
        lab = np.empty((H, W, 3), np.uint8); lab[:] = (120, 130, 140)
    elif guide_kind == "regions":
        yy, xx = np.mgrid[0:H, 0:W]
        side = (xx * H > yy * W)[..., None]
        lab = (np.where(side, np.array([60, 150, 110]), np.array([200, 120, 160])) + rng.integers(-6, 7, (H, W, 3))).astype(np.uint8)
    return np.ascontiguousarray(mask), np.ascontiguousarray(lab)
