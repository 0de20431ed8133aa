// k_region_refind.hip — re-finding a stroked object on another frame (SPEC §6.17): the step that takes a score on the tap grid (ht x wt bytes, nct_region_score's)
// and, where one is carried, the matte the sequence holds for the frame (H x W bytes), and writes the frame's matte at H x W in one pass:
//   R1  r = nct_resize_u8c1(score: ht x wt -> H x W); the target is never smaller than the grid, so the 2x area case cannot occur, and equal sizes give the byte itself
//       (the fixed-point chain with weights 2048 and 0 returns its tap: ((2048 * (128 p)) >> 16) + 2) >> 2 = p)
//   R2  confident(p) = r(p) >= 128 + margin or r(p) < 128 - margin, in integers
//   R3  out(p) = (no prior or confident(p)) ? r(p) : prior(p)
// A byte is r's or the prior's, never a mix of the two.
//
// MI355X design: the shape of k_seq_matte_warp and the finish passes. One workgroup = one 32 x 8 tile of target pixels. The score taps the tile interpolates — from the
// first pixel's source index to the last pixel's index + 1 on each axis, at most 34 x 10 bytes at a ratio >= 1 — are staged in LDS once; the arithmetic per pixel is
// resize_u8_px's (nct_pixel.h) on four LDS bytes. The prior is read and the matte stored coalesced: where W % 4 == 0 and both are dword aligned a thread takes four
// consecutive pixels, one dword load and one dword store (the workgroup is then one wave of 8 x 8 threads); else one thread per pixel and bytes. Nothing of the target's
// size is kept between R1 and R3: the pass moves 1 B in + 1 B out per pixel beside the (smaller) grid, 2 B per pixel against nct_resize_u8c1 + a select's 4 B.
// What was measured: DESIGN.md §3.22.
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_pixel.h"

#define RF_TX 32
#define RF_TY 8
#define RF_LW (RF_TX + 2)
#define RF_LH (RF_TY + 2)

// V pixels per thread along x (1 or 4); the block is (RF_TX / V) x RF_TY threads. lo = 128 - margin, hi = 128 + margin
template <int V>
__global__ __launch_bounds__(RF_TX * RF_TY / V) void k_region_refind(const uint8_t* __restrict__ score, int ht, int wt, const uint8_t* __restrict__ prior /* nullable */, int H,
                                                                     int W, int lo, int hi, uint8_t* __restrict__ out) {
    __shared__ uint8_t tile[RF_LH * RF_LW];
    const int x0 = blockIdx.x * RF_TX, y0 = blockIdx.y * RF_TY;
    const int x1 = min(x0 + RF_TX, W) - 1, y1 = min(y0 + RF_TY, H) - 1;
    // the staged region: lin_coef's index is monotonic in the coordinate; never wider than the tile's LDS
    const int sx_lo = lin_coef(x0, wt, W).s, sy_lo = lin_coef(y0, ht, H).s;
    const int tw = min(min(lin_coef(x1, wt, W).s + 1, wt - 1) - sx_lo + 1, RF_LW), th = min(min(lin_coef(y1, ht, H).s + 1, ht - 1) - sy_lo + 1, RF_LH);
    const int tid = threadIdx.y * (RF_TX / V) + threadIdx.x;
    for (int e = tid; e < tw * th; e += RF_TX * RF_TY / V) {
        const int py = e / tw, px = e - py * tw;
        tile[py * RF_LW + px] = score[(size_t)min(sy_lo + py, ht - 1) * wt + min(sx_lo + px, wt - 1)];
    }
    __syncthreads();
    const int xb = x0 + threadIdx.x * V, y = y0 + threadIdx.y;
    if (xb >= W || y >= H) return;
    const LinCoef cy = lin_coef(y, ht, H);
    const int b0 = (short)(int)rintf(cy.a0 * 2048.f), b1 = (short)(int)rintf(cy.a1 * 2048.f);
    const int ly0 = min(cy.s - sy_lo, th - 1) * RF_LW, ly1 = min(min(cy.s + 1, ht - 1) - sy_lo, th - 1) * RF_LW;
    const size_t at = (size_t)y * W + xb;
    // W % 4 == 0 and xb % 4 == 0: the four pixels are inside the row together, and the dwords are aligned where the two mattes are
    uint32_t pw = 0, packed = 0;
    if (V == 4 && prior) pw = *(const uint32_t*)(prior + at);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int x = xb + v;
        if (x >= W) break;
        const LinCoef cx = lin_coef(x, wt, W);
        const int a0 = (short)(int)rintf(cx.a0 * 2048.f), a1 = (short)(int)rintf(cx.a1 * 2048.f);
        const int lx0 = min(cx.s - sx_lo, tw - 1), lx1 = min(min(cx.s + 1, wt - 1) - sx_lo, tw - 1);
        const int p00 = tile[ly0 + lx0], p01 = tile[ly0 + lx1], p10 = tile[ly1 + lx0], p11 = tile[ly1 + lx1];
        const int r0 = cx.tail ? p00 * 2048 : p00 * a0 + p01 * a1;
        const int r1 = cx.tail ? p10 * 2048 : p10 * a0 + p11 * a1;
        int r = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
        if (prior && !(r >= hi || r < lo)) r = V == 4 ? (int)((pw >> (8 * v)) & 255u) : (int)prior[at + v];
        if (V == 1) out[at] = (uint8_t)r;
        else packed |= (uint32_t)r << (8 * v);
    }
    if (V == 4) *(uint32_t*)(out + at) = packed;
}

int nct_region_refind_check(nct_ctx* ctx, const char* who, const void* score, int ht, int wt, int H, int W, int margin, const void* out) {
    NCT_REQUIRE(score, "%s: null score", who);
    NCT_REQUIRE(out, "%s: null out", who);
    NCT_REQUIRE(ht >= 1 && ht <= 4096, "%s: ht must be in [1, 4096] (got %d)", who, ht);
    NCT_REQUIRE(wt >= 1 && wt <= 4096, "%s: wt must be in [1, 4096] (got %d)", who, wt);
    NCT_REQUIRE(H >= ht && H <= NCT_FINISH_MAX_SIDE, "%s: H must be in [ht, %d] (got %d, ht = %d)", who, NCT_FINISH_MAX_SIDE, H, ht);
    NCT_REQUIRE(W >= wt && W <= NCT_FINISH_MAX_SIDE, "%s: W must be in [wt, %d] (got %d, wt = %d)", who, NCT_FINISH_MAX_SIDE, W, wt);
    NCT_REQUIRE((long long)H * W <= NCT_FINISH_MAX_PIXELS, "%s: H * W must be at most 2^26 pixels (got %dx%d)", who, W, H);
    NCT_REQUIRE(margin >= 0 && margin <= 128, "%s: margin must be in [0, 128] (got %d)", who, margin);
    return 0;
}

static inline bool rf_overlap(const void* a, size_t na, const void* b, size_t nb) { return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; }

int nctk_region_refind(nct_ctx* ctx, hipStream_t s, const uint8_t* score, int ht, int wt, const uint8_t* prior, int H, int W, int margin, uint8_t* out) {
    NCT_TRY(nct_region_refind_check(ctx, "region_refind", score, ht, wt, H, W, margin, out));
    // a tile reads score bytes that other tiles' pixels depend on; the prior is refused with it so that `out` is never an operand
    const size_t N = (size_t)H * W;
    NCT_REQUIRE(!rf_overlap(out, N, score, (size_t)ht * wt), "region_refind: out must not overlap score");
    NCT_REQUIRE(!prior || !rf_overlap(out, N, prior, N), "region_refind: out must not overlap prior");
    const dim3 grid(cdiv(W, RF_TX), cdiv(H, RF_TY));
    if (W % 4 == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)prior & 3) == 0)
        hipLaunchKernelGGL(k_region_refind<4>, grid, dim3(RF_TX / 4, RF_TY), 0, s, score, ht, wt, prior, H, W, 128 - margin, 128 + margin, out);
    else
        hipLaunchKernelGGL(k_region_refind<1>, grid, dim3(RF_TX, RF_TY), 0, s, score, ht, wt, prior, H, W, 128 - margin, 128 + margin, out);
    NCT_LAUNCH_CHECK();
    return 0;
}
