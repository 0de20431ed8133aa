// nct_wls_plan.h — what the S2 solver (k_wls_mg.hip) decides from the shape of its grid alone: the levels of the hierarchy, which of them which kernel builds and
// cycles through, the tile shapes and the grids of the launches. Plain host C++: it knows nothing of HIP, so tests/wls_plan_check.cpp prints the plan on the CPU and
// tests/test_s2_shapes.py holds tests/s2_shapes.py's restatement against it. The shape-dependent constants of the solver are defined here, once.
#pragma once

// ---- hierarchy
constexpr int MG_COARSEST_N = 64;  // the levels are halved (rounded up) until one holds at most this many points: the coarsest grid, solved by one wave (one lane per unknown)
// The small levels of the hierarchy are built in ONE launch (k_mg_setup_tail): every level from the first one with at most MG_TAIL_N points on.
constexpr int MG_TAIL_N = 512;
constexpr int MG_MAXL = 12;        // levels a hierarchy may have (k_mg_setup_tail's LvlPack): 8193 x 8191, next to the 2^26-pixel limit of the finish, has exactly 12

// ---- the fused middle + tail of the V-cycle (k_mg_mid)
// P0 = pixels per thread of the first fused level: 1 or 2 (<= 2048 pixels: 44x44 at 700x700; 63x63 at 1000x1000 stays on tile launches — four pixels per thread measured slower)
constexpr int MID_MAXP0 = 2;      // largest first fused level, in units of 1024 pixels (1 or 2): 2 = the 44x44 level of a 700x700 pair rides in k_mg_mid (same time as its two tile launches, 186 launches fewer per pair)
static_assert(MID_MAXP0 == 1 || MID_MAXP0 == 2, "k_mg_mid is instantiated for one or two pixels per thread at its first level (four measured slower: DESIGN.md 9)");
constexpr int MID_T = 1024, MID_P1 = 1, MID_N1 = MID_T * MID_P1, MID_LV = 5;
// largest level at depth d >= 1 (the first fused level: P0 * 1024); levels shrink ~4x per depth. The levels below the first park their 10 coefficients and 4 prolongation
// weights per pixel in LDS for the way back up (a workgroup has the CU to itself: 79 KB of the 160 KB), so only right-hand side and iterate stay in registers across the recursion
constexpr int mid_cap(int d) { return d == 1 ? 1024 : (d == 2 ? 256 : 64); }

// ---- the tile-fused legs (k_mg_down / k_mg_up)
// Bandwidth-bound levels use TXB x TYB tiles; below MG_TILE_SWITCH_N pixels the legs are latency bound, so a TXS x TYS tile keeps the dependent load chains short and
// spreads over more CUs. The down leg behind the block step (X0) has one more halo pixel per side, so its big tile is 32 x 14 (41 x 23 = 943 threads).
constexpr int MG_TILE_SWITCH_N = 100000;
constexpr int TXB = 32, TYB = 16, TYB_X0 = TYB - 2;
constexpr int TXS = 16, TYS = 8;

// ---- the block step on the finest level (k_mg_block, k_mg_lines_setup): fixed blocks, aligned at 0
constexpr int LBX = 32, LBY = 16;

// What makes a plan fit the fixed arrays, so that wls_plan need not look for it:
static_assert(MG_COARSEST_N <= MG_TAIL_N, "the coarsest level is always built by k_mg_setup_tail: l_tail < nl");
static_assert(MID_LV >= 3 && mid_cap(MID_LV - 2) <= MG_COARSEST_N, "a level that fits depth MID_LV - 2 of k_mg_mid ends the hierarchy: a fused run has at most MID_LV - 1 levels");
static_assert(MID_MAXP0 * MID_T >= MG_COARSEST_N, "the coarsest level alone always fits k_mg_mid");

struct WlsLeg { int tx, ty, tiles; };                 // tile shape and number of tiles (= workgroups: the legs run on a 1-D grid) of one leg of one level
struct WlsPlan {
    int nl, H[MG_MAXL], W[MG_MAXL], n[MG_MAXL];       // the levels, finest first; n = H * W
    int l_tail;                                        // first level built by k_mg_setup_tail (levels 1 .. l_tail - 1: a launch per stage)
    int tail0, pack_nl, mid_p0;                        // levels tail0 .. nl - 1 (pack_nl of them) run in k_mg_mid<mid_p0>; levels 0 .. tail0 - 1 on tile launches
    bool big[MG_MAXL];                                 // tile-launched level l uses the TXB tiles (big[0]: the finest level does)
    WlsLeg down[MG_MAXL], up[MG_MAXL], down_x0;        // the legs of the tile-launched levels; down_x0: level 0's down leg behind the block step
    int blocks;                                        // workgroups of the block step
};

constexpr int wls_cdiv(int a, int b) { return (a + b - 1) / b; }

// The plan of an H x W grid. false: the solver refuses the grid — its hierarchy would end above MG_COARSEST_N points (only with more than MG_MAXL levels: no grid within
// the finish limits), or has a single level; nl and n[nl - 1] are set for the message.
inline bool wls_plan(int H, int W, WlsPlan& P) {
    P = WlsPlan{};
    int h = H, w = W, nl = 0;
    while (true) {
        P.H[nl] = h; P.W[nl] = w; P.n[nl] = h * w; ++nl;
        if (h * w <= MG_COARSEST_N || nl == MG_MAXL) break;
        h = (h + 1) / 2; w = (w + 1) / 2;
    }
    P.nl = nl;
    if (P.n[nl - 1] > MG_COARSEST_N || nl < 2) return false;
    P.l_tail = 1;
    while (P.n[P.l_tail] > MG_TAIL_N) ++P.l_tail;
    // The fused run: the deepest run of levels whose first has at most MID_MAXP0 * MID_T pixels and the others at most mid_cap(depth); never the fine level (its
    // right-hand side is the fp64 PCG residual and its tiles fill the chip)
    auto mid_fits = [&](int first) {
        for (int l = first; l < nl; ++l) if (P.n[l] > (l == first ? MID_MAXP0 * MID_T : mid_cap(l - first))) return false;
        return true;
    };
    P.tail0 = nl - 1;
    while (P.tail0 > 1 && mid_fits(P.tail0 - 1)) --P.tail0;
    P.pack_nl = nl - P.tail0;
    P.mid_p0 = P.n[P.tail0] <= MID_T ? 1 : 2;
    auto leg = [](int h, int w, int tx, int ty) { return WlsLeg{tx, ty, wls_cdiv(w, tx) * wls_cdiv(h, ty)}; };
    for (int l = 0; l < P.tail0; ++l) {
        P.big[l] = P.n[l] >= MG_TILE_SWITCH_N;
        P.down[l] = P.up[l] = P.big[l] ? leg(P.H[l], P.W[l], TXB, TYB) : leg(P.H[l], P.W[l], TXS, TYS);
    }
    P.down_x0 = P.big[0] ? leg(H, W, TXB, TYB_X0) : P.down[0];
    P.blocks = wls_cdiv(W, LBX) * wls_cdiv(H, LBY);
    return true;
}
