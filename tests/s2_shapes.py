"""S2's multigrid hierarchy restated and checked in Python, and the grid shapes that change which code of k_wls_mg.hip runs.
Shared by tests/test_s2_shapes.py (CPU: the mirror oracle/orc_wls_mg.c against the exact solve) and tests/test_gpu_s2_shapes.py (the kernels against the mirror).

describe(H, W) restates the solver's plan (csrc/nct_wls_plan.h: wls_plan, which mg_alloc_levels, mg_build_hierarchy, mid_levels and the launchers read) on its own;
test_s2_shapes.py::test_describe_equals_the_plan holds it and the constants below against the header, field for field. FEATURES are predicates on what it returns, so the
coverage test (test_s2_shapes.py::test_every_feature_has_a_shape) fails when a constant moves and a feature loses its last shape."""
import functools
import numpy as np

import synth
from fullres_ref import oracle_finish, smooth_ab

# The shape-dependent constants of neural-color-transfer_amd/csrc/nct_wls_plan.h, restated once:
COARSEST_N = 64        # MG_COARSEST_N — the levels are halved (rounded up) until one holds at most 64 points
MG_TAIL_N = 512        # k_mg_setup_tail builds every level from the first one with n <= 512 (l_tail)
MG_MAXL = 12           # levels a hierarchy may have (k_mg_setup_tail's LvlPack); a grid that would need more is refused
MID_LV = 5             # depths of k_mg_mid
MID_T = 1024
MID_MAXP0 = 2          # largest first fused level in units of MID_T pixels (k_mg_mid<1> / k_mg_mid<2>)
TILE_SWITCH_N = 100000  # MG_TILE_SWITCH_N — from here on a level's legs use 32x16 (up), 32x14 (level 0's down leg behind the block step) tiles, else 16x8
TXB, TYB, TYB_X0 = 32, 16, 14
TXS, TYS = 16, 8
LBX, LBY = 32, 16      # blocks of the block step (k_mg_block, k_mg_lines_setup)
FINISH_MAX_SIDE, FINISH_MAX_PIXELS = 16384, 1 << 26     # nct.h: NCT_FINISH_MAX_SIDE, NCT_FINISH_MAX_PIXELS
PAIR_SIDE = (17, 4000)  # sides of a legal pair source (nct_working_size)


def mid_cap(d):
    """`constexpr int mid_cap(int d)`: largest level at depth d >= 1 of k_mg_mid"""
    return 1024 if d == 1 else (256 if d == 2 else 64)


def _cdiv(a, b):
    return (a + b - 1) // b


def level_sizes(H, W):
    """the level loop: [(h, w)] from the finest level down, MG_MAXL of them at the most"""
    out, h, w = [], H, W
    while True:
        out.append((h, w))
        if h * w <= COARSEST_N or (h <= 8 and w <= 8) or len(out) == MG_MAXL:
            return out
        h, w = (h + 1) // 2, (w + 1) // 2


def describe(H, W):
    """What the host code of k_wls_mg.hip decides for an H x W grid. None: it refuses the grid ("wls: unsupported grid") — a single level, or still above COARSEST_N
    points at level MG_MAXL - 1."""
    lv = level_sizes(H, W)
    n = [h * w for h, w in lv]
    nl = len(lv)
    if n[-1] > COARSEST_N or nl < 2:
        return None
    l_tail = next(l for l in range(1, nl) if n[l] <= MG_TAIL_N)              # the coarsest level always qualifies

    def mid_fits(first):                                                       # mid_levels
        if nl - first > MID_LV:
            return False
        return all(n[l] <= (MID_MAXP0 * MID_T if l == first else mid_cap(l - first)) for l in range(first, nl))

    tail0 = nl - 1
    while tail0 > 1 and mid_fits(tail0 - 1):
        tail0 -= 1
    # why the level in front of the fused run stayed on tile launches: "fine" (never the fine level), "first" (above MID_MAXP0 * MID_T), "depth" (MID_LV), "cap" (a mid_cap depth binds)
    if tail0 == 1:
        stop = "fine"
    elif nl - (tail0 - 1) > MID_LV:
        stop = "depth"
    elif n[tail0 - 1] > MID_MAXP0 * MID_T:
        stop = "first"
    else:
        stop = "cap"
    big = n[0] >= TILE_SWITCH_N

    def leg(l, tx, ty):                                                        # (tile width, tile height, tiles) of a leg of level l
        return (tx, ty, _cdiv(lv[l][0], ty) * _cdiv(lv[l][1], tx))

    # per tile-launched level: (big tiles, down leg, up leg); level 0's down leg behind the block step is "down_x0"
    legs = [(True, leg(l, TXB, TYB), leg(l, TXB, TYB)) if n[l] >= TILE_SWITCH_N else (False, leg(l, TXS, TYS), leg(l, TXS, TYS)) for l in range(tail0)]
    return {"legs": legs, "down_x0": leg(0, TXB, TYB_X0) if big else leg(0, TXS, TYS),
            "H": H, "W": W, "levels": lv, "n": n, "nl": nl, "l_tail": l_tail, "tail0": tail0, "pack_nl": nl - tail0, "mid_p0": 1 if n[tail0] <= MID_T else 2, "mid_stop": stop,
            "tiles_big": big,
            "tiles_up": (_cdiv(H, TYB), _cdiv(W, TXB)), "tiles_down": (_cdiv(H, TYB_X0), _cdiv(W, TXB)),           # (tile rows, tile columns) of level 0's 32x16 / 32x14 legs
            "tiles_small": (_cdiv(H, TYS), _cdiv(W, TXS)), "blocks": (_cdiv(H, LBY), _cdiv(W, LBX))}


def _coarsened(d):
    return d["levels"][:-1]


def _legal_source(d):
    return all(PAIR_SIDE[0] <= s <= PAIR_SIDE[1] for s in (d["H"], d["W"]))


def _tile_levels(d):
    return d["levels"][1:d["tail0"]]


def _pow2(x):
    return x > 0 and x & (x - 1) == 0


def _few_tiles(d, axis):
    """>= 100 000 pixels, fewer than eight tile rows (axis 0) / columns (1) in both legs, neither tile count a multiple of 8 (mg_tile_of_block's eight bands)"""
    return d["tiles_big"] and all(t[axis] < 8 and (t[0] * t[1]) % 8 != 0 for t in (d["tiles_up"], d["tiles_down"]))


# feature name -> predicate on describe()'s result (the rows of the issue's table, one name per variant)
FEATURES = {
    "h1_level_under_17_rows": lambda d: d["H"] == 17 and _legal_source(d) and any(h == 1 for h, _ in d["levels"]),
    "w1_level_under_17_cols": lambda d: d["W"] == 17 and _legal_source(d) and any(w == 1 for _, w in d["levels"]),
    "h1_tile_launch_mid_cap_binds": lambda d: d["mid_stop"] == "cap" and any(h == 1 for h, _ in _tile_levels(d)),
    "w1_tile_launch_mid_cap_binds": lambda d: d["mid_stop"] == "cap" and any(w == 1 for _, w in _tile_levels(d)),
    "finest_1_row": lambda d: d["H"] == 1, "finest_1_col": lambda d: d["W"] == 1,
    "finest_2_rows": lambda d: d["H"] == 2, "finest_3_rows": lambda d: d["H"] == 3,
    "coarsest_1xk": lambda d: d["levels"][-1][0] == 1 and d["levels"][-1][1] > 1, "coarsest_kx1": lambda d: d["levels"][-1][1] == 1 and d["levels"][-1][0] > 1,
    "nl_2": lambda d: d["nl"] == 2,
    "all_odd": lambda d: d["nl"] > 2 and all(h & 1 and w & 1 for h, w in _coarsened(d)),
    "all_even": lambda d: d["nl"] > 2 and all(not h & 1 and not w & 1 for h, w in _coarsened(d)),
    "pow2_minus_1": lambda d: _pow2(d["H"] + 1) and _pow2(d["W"] + 1) and d["nl"] > 2,
    "mixed_parity": lambda d: any((h & 1) != (w & 1) for h, w in _coarsened(d)),
    "first_fused_le_1024": lambda d: d["mid_p0"] == 1 and d["pack_nl"] > 1,
    "first_fused_1025_2048": lambda d: d["mid_p0"] == 2,
    "nine_point_2049_4096_on_tiles": lambda d: any(2049 <= h * w <= 4096 for h, w in _tile_levels(d)),
    "pack_nl_largest": lambda d: d["pack_nl"] == MID_LV - 1,          # MID_LV itself cannot be reached: see PACK_NL_MAX
    "l_tail_1": lambda d: d["l_tail"] == 1, "l_tail_gt_1": lambda d: d["l_tail"] > 1,
    # one pixel of remainder in every tile dimension the size uses (the legs' tiles and the block step's 32 x 16 blocks)
    "below_switch_remainder_1": lambda d: 0.9 * TILE_SWITCH_N <= d["n"][0] < TILE_SWITCH_N and d["W"] % 16 == 1 and d["H"] % 8 == 1 and d["W"] % LBX == 1 and d["H"] % LBY == 1,
    "just_below_switch": lambda d: TILE_SWITCH_N - 500 <= d["n"][0] < TILE_SWITCH_N,
    "above_switch_remainder_1": lambda d: d["tiles_big"] and d["W"] % TXB == 1 and d["H"] % TYB == 1 and d["H"] % TYB_X0 == 1,
    "few_tile_rows_not_mult_8": lambda d: _few_tiles(d, 0), "few_tile_cols_not_mult_8": lambda d: _few_tiles(d, 1),
}

# pack.nl == MID_LV cannot happen: depth 3 of k_mg_mid is capped at mid_cap(3) = 64 points, and a level of at most COARSEST_N = 64 points is the last one, so a fused run
# has at most four levels and depth MID_LV - 1 never runs. test_s2_shapes.py asserts this over a sweep of grids; "pack_nl_largest" covers the deepest run there is.
PACK_NL_MAX = MID_LV - 1

# (H, W, the features the shape is there for). 17x513 is the narrowest legal source with a one-row level, 17x520 the one the upsampling and whole-pair cases use.
# 305x321 has the one-pixel remainder in the 16x8 tiles and the 32x16 blocks below the switch; 311x321 (remainders 7 and 1) is the nearest size under it.
# The sides of 17x5900 and 5900x17 are above 4000: reachable through the finish seam only.
SHAPES = [
    (17, 513, ("h1_level_under_17_rows", "coarsest_1xk")), (17, 520, ("h1_level_under_17_rows", "coarsest_1xk")), (520, 17, ("w1_level_under_17_cols", "coarsest_kx1")),
    (1, 4000, ("h1_tile_launch_mid_cap_binds", "finest_1_row", "pack_nl_largest")), (4000, 1, ("w1_tile_launch_mid_cap_binds", "finest_1_col", "pack_nl_largest")),
    (1, 130, ("finest_1_row", "coarsest_1xk")), (130, 1, ("finest_1_col", "coarsest_kx1")), (2, 300, ("finest_2_rows", "coarsest_1xk")), (3, 1000, ("finest_3_rows", "coarsest_1xk")),
    (9, 9, ("nl_2", "l_tail_1")), (16, 16, ("nl_2",)), (5, 13, ("nl_2",)),
    (33, 33, ("all_odd",)), (65, 129, ("all_odd", "l_tail_gt_1")), (32, 32, ("all_even", "l_tail_1", "first_fused_le_1024")), (64, 128, ("all_even", "first_fused_1025_2048")),
    (31, 31, ("pow2_minus_1",)), (33, 64, ("mixed_parity", "first_fused_le_1024")),
    (100, 141, ("nine_point_2049_4096_on_tiles",)),
    (305, 321, ("below_switch_remainder_1",)), (311, 321, ("just_below_switch",)), (337, 321, ("above_switch_remainder_1",)),
    (17, 5900, ("few_tile_rows_not_mult_8",)), (5900, 17, ("few_tile_cols_not_mult_8",)),
]
HW = [(H, W) for H, W, _ in SHAPES]
# one, two or three pixels high or wide, and the legal sources with a one-pixel level: the second pass (flat sources), the block step off, the split solve
THIN = [(H, W) for H, W in HW if min(H, W) <= 3 or (H, W) in ((17, 520), (520, 17))]
# grids the solver refuses (64 points or fewer)
REFUSED = [(8, 8), (1, 64), (4, 16), (1, 1)]
# No grid within the finish limits needs more than MG_MAXL levels, so none is refused for its level count: level 11 of an H x W grid holds at most
# (H / 2048 + 1) (W / 2048 + 1) <= 2^26 / 2^22 + (16384 + 4096) / 2048 + 1 = 27 points, under COARSEST_N. Exactly MG_MAXL levels — k_mg_setup_tail's LvlPack filled to its
# last slot — are reached only next to the pixel limit: 8193 x 8191 ends 9x8 (72 points), 5x4. test_s2_shapes.py asserts this on the list below; none of it is solved.
EXTREMES = [(16384, 4096), (4096, 16384), (16384, 1), (1, 16384), (16383, 4095), (8192, 8192), (8193, 8191), (8191, 8193)]

S2_RTOL, S2_ATOL = 2e-5, 2e-6          # the project's S2 bound (test_gpu_vs_ref64._check_after_s1)
# Largest |mirror - exact| / (S2_ATOL + S2_RTOL |exact|) over every case of test_s2_shapes.py (both sources, the block step on and off, the upsampling cases), measured
# from the mirror: MIRROR_DEV_MEASURED. The GPU equals the mirror bit for bit, so the figure is the GPU's; the factor 4 absorbs another input seed, not other arithmetic.
MIRROR_DEV_MEASURED = 0.00187       # 17x520, flat source, block step off; 0.00177 at 5900x17 with it
MIRROR_DEV_BOUND = 4 * MIRROR_DEV_MEASURED

# upsampling calls where U1 reads a level grid of one or two rows / one column: (level grid, target)
UPSAMPLE = [((2, 33), (17, 520)), ((1, 8), (17, 130)), ((5, 1), (130, 17))]


def source(kind, seed, H, W):
    """kind "cos": synth.image; "flat": synth.image_flat, whose flat rectangle and posterised band are empty on a grid under 8 rows — there the image is made W x H and
    transposed, so the runs of one colour (coupling contrasts of 10^4: what the block step is for) lie along the long side"""
    if kind == "cos":
        return synth.image(seed, H, W)
    if H < 8:
        return np.ascontiguousarray(synth.image_flat(seed, W, H).transpose(1, 0, 2))
    return synth.image_flat(seed, H, W)


@functools.lru_cache(maxsize=None)
def case_inputs(H, W, kind="cos", level=None):
    """(ab [2][h*w][3], (h, w), s_full) of a shape, shared and not to be written to; level None: the equal-size call"""
    h, w = level or (H, W)
    seed = 1000 * H + W + (7 if kind == "flat" else 0)
    return smooth_ab(seed, h, w), (h, w), source(kind, seed + 1, H, W)


@functools.lru_cache(maxsize=None)
def mirror(oracle, H, W, kind="cos", lines=True, level=None):
    """oracle_finish of case_inputs (working size = the target, so only the equal-size call takes the x4 branch) -> (bgr, stages); lines False: without the block step"""
    ab, (h, w), s = case_inputs(H, W, kind, level)
    oracle.l.orc_set_mg_lines(1 if lines else 0)
    try:
        return oracle_finish(oracle, ab, h, w, H, W, s)
    finally:
        oracle.l.orc_set_mg_lines(1)


def s2_lambda(H, W, h, w, lambda_init=0.024):
    return lambda_init * (H * W) / (h * w) * (4 if (h, w) == (H, W) else 1)


def bound_units(got, exact):
    """largest |got - exact| in units of the S2 bound"""
    return float((np.abs(got - exact) / (S2_ATOL + S2_RTOL * np.abs(exact))).max())
