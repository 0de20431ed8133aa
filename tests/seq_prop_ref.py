"""Propagated frames of a sequence (SPEC §6.5): the warp (rule 3) restated in numpy, a propagated frame composed from the oracle's exported stages and seq_mc_ref's
search (rules 1-5), and sequences that alternate full and propagated frames on a key-frame grid. Shared by tests/test_seq_prop.py (CPU) and
tests/test_gpu_seq_prop.py. The warp moves 64-bit words: a NaN comes through with its payload."""
import numpy as np

import fullres_ref
import multi_ref
import seq_mc_ref
import seq_ref


def warp(x_prev, field):
    """rule 3: x_prev [2][h*w][3] doubles, field int16 [h][w][2] of (my, mx) -> x_prev read at p + m(p), a vector that leaves the grid clamped component-wise first"""
    f = np.asarray(field, np.int16).astype(np.int64)
    h, w = f.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    src = (np.clip(yy + f[..., 0], 0, h - 1) * w + np.clip(xx + f[..., 1], 0, w - 1)).reshape(-1)
    words = np.ascontiguousarray(x_prev, np.float64).reshape(2, h * w, 3).view(np.uint64)
    return np.ascontiguousarray(words[:, src, :]).view(np.float64)


def frame_propagate(orc, src, state, mot=None, levels=5):
    """one propagated frame. state: the list per level of (X', L) the previous frame (full or propagated) returned; mot: (radius0, radius, penalty) or None / both radii 0
    = motion off. -> (result, keep, new state); keep: per level "ab_blend" (X'_t), "motion", "tau_map" (ones)"""
    assert state is not None and len(state) == levels
    src = np.ascontiguousarray(src, np.uint8)
    H, W = src.shape[:2]
    simg = multi_ref.pyramid(orc, src)
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    keep = {k: [] for k in ("ab_blend", "motion", "tau_map")}
    new_state = []
    field = None
    for l in range(levels):
        ah, aw = simg[l].shape[:2]
        L = orc.bgr2lab(simg[l])
        if on:
            m = field = seq_mc_ref.motion(L, state[l][1], field, mot[0] if l == 0 else mot[1], mot[2])
            X = warp(state[l][0], m)
        else:
            m = np.zeros((ah, aw, 2), np.int16)
            X = np.asarray(state[l][0], np.float64).reshape(2, ah * aw, 3)
        new_state.append((X, L))
        keep["ab_blend"].append(X); keep["motion"].append(m); keep["tau_map"].append(np.ones((ah, aw)))
    ah, aw = simg[levels - 1].shape[:2]
    out, _ = fullres_ref.oracle_finish(orc, new_state[-1][0], ah, aw, H, W, src)
    return out, keep, new_state


def is_key(k, key):
    """the k-th frame since the sequence began is a full frame iff k % key == 0"""
    return k % key == 0


def sequence_keyed(orc, frames, ref, ws, bs, key=None, full=None, tau=seq_ref.TAU, sigma=seq_ref.SIGMA, mot=(seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY), levels=5):
    """full frames (seq_mc_ref.frame) on the key-frame grid `key`, or where the list of booleans `full` says so, propagated frames elsewhere
    -> (list of results, list of keeps, list of "was a full frame")"""
    R = seq_ref.prepare_reference(orc, ref, ws, bs)
    plan = [is_key(k, key) for k in range(len(frames))] if full is None else list(full)
    assert plan[0]
    state, outs, keeps = None, [], []
    for f, whole in zip(frames, plan):
        if whole:
            out, keep, state = seq_mc_ref.frame(orc, f, R, ws, bs, state, tau, sigma, mot=mot, levels=levels)
        else:
            out, keep, state = frame_propagate(orc, f, state, mot=mot, levels=levels)
        outs.append(out); keeps.append(keep)
    return outs, keeps, plan


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def warp_case(h, w, seed, kind="random"):
    """-> (x_prev [2][h*w][3], field int16 [h][w][2]). kinds: "random" (vectors in +-3: on small grids many leave it), "outside" (vectors far outside the grid in every
    direction, the int16 extremes among them), "nan" (random vectors, NaN words with distinct payloads and both signs in the map)"""
    rng = np.random.default_rng(seed)
    n = h * w
    x = np.stack([1.0 + 0.3 * rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3))])
    if kind == "outside":
        field = rng.integers(-3 * max(h, w) - 5, 3 * max(h, w) + 6, (h, w, 2)).astype(np.int16)
        field.reshape(-1, 2)[::3] = rng.choice(np.array([-32768, 32767, 0], np.int16), (len(field.reshape(-1, 2)[::3]), 2))
    else:
        field = rng.integers(-3, 4, (h, w, 2)).astype(np.int16)
    if kind == "nan":
        u = x.view(np.uint64).reshape(-1)
        idx = np.arange(0, u.size, 5)
        u[idx] = np.uint64(0x7FF8000000000000) | (idx.astype(np.uint64) + np.uint64(1))            # quiet NaNs, payload = position + 1
        u[idx[::2]] |= np.uint64(0x8000000000000000)
        u[idx[::3]] = np.uint64(0x7FF0000000000000) | (idx[::3].astype(np.uint64) + np.uint64(1))  # signalling ones
    return x, field


WARP_GRIDS = [g for g, _ in seq_ref.BLEND_CASES] + [(37, 70)]
