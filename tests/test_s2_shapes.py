"""S2 on the grid shapes that change its hierarchy (tests/s2_shapes.py), on the CPU: the shape list covers every feature according to describe(), and the mirror
(oracle/orc_wls_mg.c, which the kernels must equal bit for bit: tests/test_gpu_s2_shapes.py) solves the system at every one of them — against the exact float64
solve within the project's S2 bound and within s2_shapes.MIRROR_DEV_BOUND, four times the largest deviation measured here."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import nct
import ref64
import s2_shapes as S
from fullres_ref import s2_levels

ALPHA = 1.2


def test_describe_restates_the_known_hierarchies():
    """sizes the suite already runs, worked out by hand from k_wls_mg.hip's comments (44x44 of a 700x700 pair rides in k_mg_mid<2>, 63x63 of 1000x1000 stays on tiles)"""
    d = S.describe(700, 700)
    assert d["levels"] == [(700, 700), (350, 350), (175, 175), (88, 88), (44, 44), (22, 22), (11, 11), (6, 6)]
    assert (d["nl"], d["l_tail"], d["tail0"], d["pack_nl"], d["mid_p0"], d["tiles_big"]) == (8, 5, 4, 4, 2, True)
    d = S.describe(1000, 1000)
    assert d["levels"][4:] == [(63, 63), (32, 32), (16, 16), (8, 8)] and (d["tail0"], d["mid_p0"], d["mid_stop"]) == (5, 1, "first")
    d = S.describe(17, 520)
    assert d["levels"] == [(17, 520), (9, 260), (5, 130), (3, 65), (2, 33), (1, 17)]
    assert S.describe(17, 400)["levels"][-1] == (2, 25) and S.describe(17, 512)["levels"][-1] == (2, 32)
    d = S.describe(1, 4000)
    assert d["n"] == [4000, 2000, 1000, 500, 250, 125, 63] and (d["tail0"], d["pack_nl"], d["mid_stop"]) == (3, 4, "cap")
    for H, W in S.HW + [(700, 700), (3000, 3000)]:
        assert S.describe(H, W)["nl"] == s2_levels(H, W)
    for H, W in S.REFUSED:
        assert S.describe(H, W) is None


def test_every_feature_has_a_shape():
    """by describe()'s output, not by the label: every feature has a shape, and every label is true"""
    for H, W, labels in S.SHAPES:
        d = S.describe(H, W)
        assert d is not None, (H, W)
        print(f"{H}x{W}: levels {d['levels']} nl {d['nl']} l_tail {d['l_tail']} tail0 {d['tail0']} pack.nl {d['pack_nl']} k_mg_mid<{d['mid_p0']}> stop {d['mid_stop']} "
              f"big tiles {d['tiles_big']} up {d['tiles_up']} down {d['tiles_down']} 16x8 {d['tiles_small']}: {[k for k, f in S.FEATURES.items() if f(d)]}")
        for k in labels:
            assert S.FEATURES[k](d), (H, W, k)
    for k, f in S.FEATURES.items():
        assert any(f(S.describe(H, W)) for H, W in S.HW), f"no shape of SHAPES shows {k}"
    # the thin subset holds what the second pass, the block-step-off pass and the split solve are for
    thin = [k for k in S.FEATURES if k.startswith(("finest_", "h1_", "w1_", "coarsest_"))]
    for k in thin:
        assert any(S.FEATURES[k](S.describe(H, W)) for H, W in S.THIN), k
    # the two seam-only shapes really are outside a pair's sides, everything under "legal source" inside
    assert max(S.HW[-1]) > S.PAIR_SIDE[1] and max(S.HW[-2]) > S.PAIR_SIDE[1]
    # the upsampling cases read the coarsest levels of their targets' hierarchies (or a grid of one row / column)
    assert S.describe(17, 520)["levels"][4] == (2, 33) and [lv for lv, _ in S.UPSAMPLE] == [(2, 33), (1, 8), (5, 1)]


def _plan_lines(tmp_path, grids):
    """tests/wls_plan_check.cpp under AddressSanitizer + UBSan on `grids` -> (the header's constants {name: text}, [the words of each grid's line])"""
    exe = str(tmp_path / "wls_plan_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(nct.PKG_ROOT, "csrc"),
                        os.path.join(os.path.dirname(__file__), "wls_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], input="".join(f"{H} {W}\n" for H, W in grids), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0][0] == "const" and len(lines) == 1 + len(grids)
    return dict(w.split("=") for w in lines[0][1:]), lines[1:]


def _describe_words(H, W):
    """describe(H, W) in the words of wls_plan_check's line"""
    d = S.describe(H, W)
    if d is None:
        lv = S.level_sizes(H, W)
        return [str(H), str(W), "refused", f"nl={len(lv)}", f"coarsest={lv[-1][0] * lv[-1][1]}"]
    assert len(d["legs"]) == d["tail0"] and d["legs"][0][0] == d["tiles_big"] and d["n"] == [h * w for h, w in d["levels"]]
    # the (rows, columns) forms the features read are the same legs
    up0 = d["tiles_up"] if d["tiles_big"] else d["tiles_small"]
    down0 = d["tiles_down"] if d["tiles_big"] else d["tiles_small"]
    assert d["legs"][0][2][2] == up0[0] * up0[1] and d["down_x0"][2] == down0[0] * down0[1]
    leg = "{}={}x{}:{}".format
    out = [str(H), str(W), f"nl={d['nl']}", "levels=" + ",".join(f"{h}x{w}:{h * w}" for h, w in d["levels"]), f"l_tail={d['l_tail']}", f"tail0={d['tail0']}",
           f"pack_nl={d['pack_nl']}", f"mid_p0={d['mid_p0']}", f"blocks={d['blocks'][0] * d['blocks'][1]}", leg("down_x0", *d["down_x0"])]
    for big, down, up in d["legs"]:
        out += [f"big={int(big)}", leg("down", *down), leg("up", *up)]
    return out


def test_describe_equals_the_plan(tmp_path):
    """the constants of s2_shapes.py and describe(H, W) against csrc/nct_wls_plan.h — what k_wls_mg.hip reads — field for field: every grid up to 96 x 96, the shape lists,
    the two benchmark sizes and 500 sizes drawn inside the finish limits. None of them is refused for its level count, none has a fused run of MID_LV levels."""
    rng = random.Random(20240611)
    drawn = []
    while len(drawn) < 500:                                 # sides log-uniform in [1, FINISH_MAX_SIDE], the pixel limit applied
        H, W = (int(round(2 ** rng.uniform(0, 14))) for _ in range(2))
        if H * W <= S.FINISH_MAX_PIXELS:
            drawn.append((H, W))
    grids = [(H, W) for H in range(1, 97) for W in range(1, 97)] + S.HW + S.EXTREMES + S.REFUSED + [t for _, t in S.UPSAMPLE] + [lv for lv, _ in S.UPSAMPLE]
    grids += [(700, 700), (1000, 1000)] + drawn
    const, lines = _plan_lines(tmp_path, grids)
    mine = {"COARSEST_N": S.COARSEST_N, "MG_TAIL_N": S.MG_TAIL_N, "MG_MAXL": S.MG_MAXL, "MID_LV": S.MID_LV, "MID_T": S.MID_T, "MID_MAXP0": S.MID_MAXP0,
            "TILE_SWITCH_N": S.TILE_SWITCH_N, "TXB": S.TXB, "TYB": S.TYB, "TYB_X0": S.TYB_X0, "TXS": S.TXS, "TYS": S.TYS, "LBX": S.LBX, "LBY": S.LBY,
            "mid_cap": ",".join(str(S.mid_cap(d)) for d in (1, 2, 3, 4))}
    for k, v in mine.items():
        assert const[k] == str(v), (k, const[k], v)
    assert max(H for H, _ in drawn) > 4000 and sum(H * W >= S.TILE_SWITCH_N for H, W in drawn) > 100 and sum(H * W < S.TILE_SWITCH_N for H, W in drawn) > 100
    for (H, W), words in zip(grids, lines):
        assert words == _describe_words(H, W), (H, W)
        d = S.describe(H, W)
        if d is None:
            assert H * W <= S.COARSEST_N, (H, W)            # refused for a single level, never for the level count
        else:
            assert d["nl"] <= S.MG_MAXL and d["pack_nl"] < S.MID_LV, (H, W)


def test_no_accepted_grid_reaches_the_deep_branches():
    """within the finish limits no hierarchy needs more than MG_MAXL levels (so the refusal of deeper hierarchies meets no accepted size; 8193 x 8191 has exactly
    MG_MAXL), and no fused run has MID_LV levels (depth 3 is capped at 64 points, which ends the hierarchy): described only, not solved"""
    for H, W in S.EXTREMES:
        assert H <= S.FINISH_MAX_SIDE and W <= S.FINISH_MAX_SIDE and H * W <= S.FINISH_MAX_PIXELS
        d = S.describe(H, W)
        print(H, W, d["nl"], d["n"])
        assert d["nl"] <= S.MG_MAXL and d["l_tail"] < d["nl"] and d["n"][-1] <= S.COARSEST_N
    assert S.describe(8193, 8191)["nl"] == S.MG_MAXL and S.describe(16384, 4096)["nl"] == 11 and S.describe(16384, 1)["nl"] == 9
    sides = sorted(set(list(range(1, 70)) + [2 ** k + e for k in range(6, 15) for e in (-1, 0, 1) if 2 ** k + e <= S.FINISH_MAX_SIDE] + [100, 141, 700, 1000, 4000, 5900]))
    worst = 0
    for H in sides:
        for W in sides:
            if H * W > S.FINISH_MAX_PIXELS:
                continue
            d = S.describe(H, W)
            if d is None:
                assert H * W <= S.COARSEST_N
                continue
            assert d["nl"] <= S.MG_MAXL and 1 <= d["pack_nl"] <= S.PACK_NL_MAX and d["n"][d["tail0"]] <= S.MID_MAXP0 * S.MID_T
            assert all(n <= S.mid_cap(l - d["tail0"]) for l, n in enumerate(d["n"]) if l > d["tail0"])
            worst = max(worst, d["pack_nl"])
    assert worst == S.PACK_NL_MAX == S.MID_LV - 1


def test_flat_sources_of_thin_shapes_hold_runs():
    """the second pass is there for runs of one colour along the thin grid: each thin flat source has eight equal neighbour pairs in a row somewhere (a run of nine
    pixels: couplings of lamda / 1e-4 inside it, 10^4 times smaller at its ends)"""
    for H, W in S.THIN:
        s = S.source("flat", 5, H, W)
        assert s.shape == (H, W, 3)
        eq = np.all(s[:, 1:] == s[:, :-1], axis=2) if W >= H else np.all(s[1:] == s[:-1], axis=2).T
        run = max(len(r) for row in eq for r in "".join("1" if v else "0" for v in row).split("0"))
        assert run >= 8, (H, W, run)


@functools.lru_cache(maxsize=None)
def _check_mirror(oracle, H, W, kind, lines, level=None):
    """the mirror's stages against ref64 -> (deviation in units of the S2 bound, iteration counts)"""
    _, exp = S.mirror(oracle, H, W, kind, lines, level)
    ab, (h, w), s = S.case_inputs(H, W, kind, level)
    flab = oracle.bgr2lab(s).reshape(-1, 3) / 255.0
    if level is None:
        assert np.array_equal(exp["ab_up"], ab)
    assert np.array_equal(exp["roughness"], ref64.roughness(exp["ab_up"], flab))
    exact = ref64.wls_solve_exact(exp["ab_up"], flab, H, W, S.s2_lambda(H, W, h, w), ALPHA, exp["roughness"])
    dev = S.bound_units(exp["ab_wls"], exact)
    d = S.describe(H, W)
    print(f"s2-shape {H}x{W} {kind} lines={int(lines)} level={level}: levels {d['levels']} nl {d['nl']} tail0 {d['tail0']} iters {exp['wls_iters'].tolist()} dev {dev:.3g} of the S2 bound")
    assert np.allclose(exp["ab_wls"], exact, rtol=S.S2_RTOL, atol=S.S2_ATOL)
    assert min(exp["wls_iters"]) > 0                 # six non-zero right-hand sides, none solved by its initial guess (oracle_finish has asserted convergence)
    return dev


def _cases():
    out = [(H, W, "cos", True, None) for H, W in S.HW]
    out += [(H, W, "flat", True, None) for H, W in S.THIN]
    out += [(H, W, kind, False, None) for H, W in S.THIN for kind in ("cos", "flat")]
    out += [(H, W, "cos", True, lv) for lv, (H, W) in S.UPSAMPLE]
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-lines{int(c[3])}" + (f"-from{c[4][0]}x{c[4][1]}" if c[4] else ""))
def test_mirror_solves_the_system(oracle, case):
    """oracle_finish against ref64.wls_solve_exact: the project's bound, the roughness equal, and the tighter measured bound (test_mirror_deviation_constant_is_the_measured_one
    ties MIRROR_DEV_MEASURED to what is measured here)"""
    dev = _check_mirror(oracle, *case)
    assert dev <= S.MIRROR_DEV_BOUND, (case, dev)


def test_mirror_deviation_constant_is_the_measured_one(oracle):
    """MIRROR_DEV_MEASURED is the largest deviation over the cases above (cached: nothing is solved twice), to its two printed digits"""
    worst = max(_check_mirror(oracle, *c) for c in _cases())
    print("s2-shape worst deviation %.3g of the S2 bound" % worst)
    assert worst <= S.MIRROR_DEV_MEASURED * 1.05 and worst >= S.MIRROR_DEV_MEASURED * 0.8
