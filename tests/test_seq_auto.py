"""Adaptive key frames (SPEC §6.7) without a GPU: the numpy measure against a scalar loop, the decision's edge cases, and the plans of the three clips the GPU tests run,
asserted on the reference alone (tests/seq_auto_ref.py) so that the conditions those tests rely on are known to hold."""
import numpy as np
import pytest

import seq_auto_ref as ar
import seq_ref


def change_scalar(L, Lp, field, T):
    """rule 1 pixel by pixel"""
    h, w = L.shape[:2]
    sad = changed = 0
    for y in range(h):
        for x in range(w):
            ty, tx = y, x
            if field is not None:
                ty = min(max(y + int(field[y, x, 0]), 0), h - 1)
                tx = min(max(x + int(field[y, x, 1]), 0), w - 1)
            r = sum(abs(int(L[y, x, c]) - int(Lp[ty, tx, c])) for c in range(3))
            sad += r
            changed += r > T
    return {"sad": sad, "changed": changed, "pixels": h * w}


GRIDS = sorted({g for g, _ in seq_ref.BLEND_CASES})


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("field", ["field", "none", "outside"])
def test_numpy_measure_equals_the_scalar_loop(grid, field):
    h, w = grid
    for kind in ("random", "equal", "noise"):
        L, Lp, m = ar.change_case(h, w, 17 * h + w, kind, field)
        if field == "outside" and h * w > 1:
            yy, xx = np.mgrid[0:h, 0:w]
            f = m.astype(np.int64)
            assert ((yy + f[..., 0] < 0) | (yy + f[..., 0] >= h) | (xx + f[..., 1] < 0) | (xx + f[..., 1] >= w)).any()      # the clamp is at work
        for T in (0, 24, 765):
            assert ar.change(L, Lp, m, T) == change_scalar(L, Lp, m, T), (kind, T)
        if kind == "equal" and field == "none":
            assert ar.change(L, Lp, m, 0) == {"sad": 0, "changed": 0, "pixels": h * w}
        assert ar.change(L, Lp, m, 765)["changed"] == 0                                                                  # r <= 765: nothing is over the largest threshold


def test_measure_extremes():
    L, Lp = np.zeros((3, 5, 3), np.uint8), np.full((3, 5, 3), 255, np.uint8)
    assert ar.change(L, Lp, None, 764) == {"sad": 765 * 15, "changed": 15, "pixels": 15}
    assert ar.change(L, Lp, None, 765)["changed"] == 0


def test_decision_edges():
    c = lambda changed, pixels=1000: {"sad": 0, "changed": changed, "pixels": pixels}
    P, K, X = ar.PROPAGATED, ar.KEYFRAME, ar.SCENE_CUT
    # equality at the cut threshold: changed * 1000 >= cut * pixels
    assert ar.decide(c(500), 0, 0, cut=500, key=ar.NEVER, max_gap=1000) == X
    assert ar.decide(c(499), 0, 0, cut=500, key=ar.NEVER, max_gap=1000) == P
    # equality at the key threshold, through the accumulated count
    assert ar.decide(c(40), 60, 0, cut=ar.NEVER, key=100, max_gap=1000) == K
    assert ar.decide(c(39), 60, 0, cut=ar.NEVER, key=100, max_gap=1000) == P
    assert ar.decide(c(100), 0, 0, cut=ar.NEVER, key=100, max_gap=1000) == K
    # the cut is looked at first
    assert ar.decide(c(500), 0, 0, cut=500, key=100, max_gap=1) == X
    # 0: always (even a frame that did not change), 1001: never (even a frame that changed everywhere)
    assert ar.decide(c(0), 0, 0, cut=0, key=ar.NEVER, max_gap=1000) == X
    assert ar.decide(c(0), 0, 0, cut=ar.NEVER, key=0, max_gap=1000) == K
    assert ar.decide(c(1000), 10 ** 9, 0, cut=ar.NEVER, key=ar.NEVER, max_gap=1000) == P
    assert ar.decide(c(1000), 0, 0, cut=1000, key=ar.NEVER, max_gap=1000) == X
    # max_gap 1: every frame is full; max_gap N: N - 1 propagated frames between two full ones
    assert ar.decide(c(0), 0, 0, cut=ar.NEVER, key=ar.NEVER, max_gap=1) == K
    for gap in range(6):
        assert ar.decide(c(0), 0, gap, cut=ar.NEVER, key=ar.NEVER, max_gap=4) == (K if gap >= 3 else P)
    # the largest grid and count stay exact
    assert ar.decide(c(2 ** 24 - 1, 2 ** 24), 0, 0, cut=1000, key=ar.NEVER, max_gap=1000) == P
    assert ar.decide(c(2 ** 24, 2 ** 24), 0, 0, cut=1000, key=ar.NEVER, max_gap=1000) == X


@pytest.fixture(scope="module")
def plans(oracle):
    return {name: ar.plan(oracle, frames, 5, mot, auto) for name, (frames, mot, auto) in ar.clips().items()}


def test_plan_of_the_pan(plans):
    p = plans["pan"]
    print("pan:", ar.kinds(p), [(d["changed"], d["pixels"]) for d in p])
    assert p[0]["kind"] == ar.FIRST and p[0]["level"] == -1 and p[0]["changed"] == 0
    assert all(d["level"] == 2 and d["pixels"] == 14 * 16 for d in p[1:])
    assert ar.PROPAGATED in [d["kind"] for d in p] and ar.KEYFRAME in [d["kind"] for d in p] and ar.SCENE_CUT not in [d["kind"] for d in p]
    # the key frame is one the accumulated count asked for, not max_gap and not a single frame's count: the sum is at work
    k = [d for d in p if d["kind"] == ar.KEYFRAME][0]
    assert k["gap"] < 7 and k["acc_changed"] > 0 and k["changed"] * 1000 < 60 * k["pixels"]


def test_plan_with_motion_off(plans):
    p = plans["motion_off"]
    print("motion off:", ar.kinds(p), [(d["changed"], d["pixels"]) for d in p])
    assert ar.kinds(p) == "FKKKK"
    assert all(100 * d["pixels"] <= d["changed"] * 1000 < 500 * d["pixels"] for d in p[1:])


def test_plan_of_the_cut(plans):
    p = plans["cut"]
    print("cut:", ar.kinds(p), [(d["changed"], d["pixels"]) for d in p])
    assert ar.kinds(p) == "FPCP"
    assert p[3]["gap"] == 0 and p[3]["acc_changed"] == 0                                        # the cut started the count over


def test_identities_of_the_plan(oracle):
    frames, mot, _ = ar.clips()["pan"]
    assert ar.kinds(ar.plan(oracle, frames, 5, mot, (24, ar.NEVER, 0, 8))) == "FKKKK"             # (c) the all-full sequence
    assert ar.kinds(ar.plan(oracle, frames, 5, mot, (24, ar.NEVER, ar.NEVER, 3))) == "FPPKP"      # (d) the grid of -key 3
    same = [frames[0], frames[0], frames[0]]
    p = ar.plan(oracle, same, 5, mot, (0, ar.NEVER, ar.NEVER, 8))                                # (e) an identical frame: nothing changed, even at T = 0
    assert all(d["sad"] == 0 and d["changed"] == 0 for d in p[1:])
    assert [ar.probe_level(n) for n in (1, 2, 3, 4, 5)] == [0, 1, 2, 2, 2]
