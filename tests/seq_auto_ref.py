"""Adaptive key frames (SPEC §6.7): the change measure (rule 1) restated in numpy on int64, the probe (rule 2) composed from the oracle's pyramid and Lab conversion and
seq_mc_ref's search, the decision (rule 3) and the plan of a whole clip. Shared by tests/test_seq_auto.py (CPU) and tests/test_gpu_seq_auto.py. L_t is the frame's own
pyramid in 8-bit Lab, so nothing here needs VGG19 or the colour stage. Everything is integer arithmetic."""
import numpy as np

import multi_ref
import seq_mc_ref

THRESHOLD, CUT, KEY, MAX_GAP = 24, 500, 100, 8          # nct_seq_auto_default
FIRST, PROPAGATED, KEYFRAME, SCENE_CUT = 0, 1, 2, 3     # NCT_SEQ_*
NEVER = 1001


def change(L, Lp, field, T):
    """rule 1: L, Lp h x w x 3 uint8 (frame t, frame t-1), field None (m = 0) or int16 [h][w][2] of (my, mx), a vector that leaves the grid clamped component-wise first
    -> {"sad", "changed", "pixels"}"""
    L = np.asarray(L, np.uint8).astype(np.int64); Lp = np.asarray(Lp, np.uint8).astype(np.int64)
    h, w = L.shape[:2]
    if field is not None:
        f = np.asarray(field, np.int16).astype(np.int64).reshape(h, w, 2)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
        Lp = Lp[np.clip(yy + f[..., 0], 0, h - 1), np.clip(xx + f[..., 1], 0, w - 1)]
    r = np.abs(L - Lp).sum(axis=2)
    return {"sad": int(r.sum()), "changed": int((r > T).sum()), "pixels": h * w}


def probe_level(levels):
    return min(levels - 1, 2)


def labs(orc, frame, levels):
    """L_t[l] for l = 0 … lambda: what the probe needs of a frame, and what a frame leaves of itself in the state for the next probe"""
    simg = multi_ref.pyramid(orc, frame)
    return [orc.bgr2lab(simg[l]) for l in range(probe_level(levels) + 1)]


def probe(cur, prev, mot, T):
    """rule 2 on two frames' labs(): with mot = (radius0, radius, penalty) the fields of SPEC §6.4 rules 1-3 level by level down the parent chain, then rule 1 at the last
    level; mot None or both radii 0: no field"""
    on = mot is not None and (mot[0] > 0 or mot[1] > 0)
    field = None
    if on:
        for l in range(len(cur)):
            field = seq_mc_ref.motion(cur[l], prev[l], field, mot[0] if l == 0 else mot[1], mot[2])
    return change(cur[-1], prev[-1], field, T)


def decide(c, acc, gap, cut=CUT, key=KEY, max_gap=MAX_GAP):
    """rule 3 on a measured frame (a frame of a sequence without state is FIRST and never comes here); Python integers do not overflow. 1001 is "never": for the cut
    the comparison says so by itself (changed <= pixels), for the key it is said apart, since the accumulated count may exceed the pixels"""
    if c["changed"] * 1000 >= cut * c["pixels"]:
        return SCENE_CUT
    if gap >= max_gap - 1 or (key != NEVER and (acc + c["changed"]) * 1000 >= key * c["pixels"]):
        return KEYFRAME
    return PROPAGATED


def plan(orc, frames, levels, mot, auto):
    """walk a clip as nct_seq_frame_auto does. auto = (threshold, cut_permille, key_permille, max_gap) -> list of dicts per frame: "kind", "level", "sad", "changed",
    "pixels", "acc_changed", "gap" (the counters before the frame's update)"""
    T, cut, key, max_gap = auto
    out, prev, acc, gap = [], None, 0, 0
    for f in frames:
        cur = labs(orc, f, levels)
        if prev is None:
            d = {"kind": FIRST, "level": -1, "sad": 0, "changed": 0, "pixels": 0}
        else:
            d = probe(cur, prev, mot, T)
            d["kind"] = decide(d, acc, gap, cut, key, max_gap); d["level"] = probe_level(levels)
        d["acc_changed"] = acc; d["gap"] = gap
        if d["kind"] == PROPAGATED:
            acc += d["changed"]; gap += 1
        else:
            acc = gap = 0
        out.append(d)
        prev = cur
    return out


def kinds(p):
    return "".join("FPKC"[d["kind"]] for d in p)


def change_case(h, w, seed, kind="random", field="field"):
    """-> (L, Lp, field or None). kinds: "random" (Lp = L with small differences in most places and a large one in a patch: pixels on both sides of a threshold), "equal",
    "noise" (two unrelated maps). field: "field" (vectors in +-3), "none", "outside" (vectors far outside the grid, the int16 extremes among them)"""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "equal":
        Lp = L.copy()
    elif kind == "noise":
        Lp = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        Lp = np.clip(L.astype(int) + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        Lp[h // 3:h // 3 + max(1, h // 4), w // 3:w // 3 + max(1, w // 4)] = rng.integers(0, 256, 3, dtype=np.uint8)
    if field == "none":
        m = None
    elif field == "outside":
        m = rng.integers(-3 * max(h, w) - 5, 3 * max(h, w) + 6, (h, w, 2)).astype(np.int16)
        m.reshape(-1, 2)[::3] = rng.choice(np.array([-32768, 32767, 0], np.int16), (len(m.reshape(-1, 2)[::3]), 2))
    else:
        m = rng.integers(-3, 4, (h, w, 2)).astype(np.int16)
    return L, Lp, m


# ---- the three clips of the tests: (frames, motion, auto)

def clips(h=56, w=64):
    import seq_ref
    pan = seq_ref.pan_frames(5, h, w, step=4)
    a = seq_ref.pan_frames(3, h, w, step=4)
    b = seq_ref.pan_frames(3, h, w, step=4, seed=2000)
    mot = (seq_mc_ref.RADIUS0, seq_mc_ref.RADIUS, seq_mc_ref.PENALTY)
    auto = (24, 500, 60, 8)
    return {"pan": (pan, mot, auto), "motion_off": (pan, None, auto), "cut": ([a[0], a[1], b[0], b[1]], mot, auto)}
