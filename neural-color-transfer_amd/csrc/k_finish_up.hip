// k_finish_up.hip — the upsampling finish (SPEC §6.8): the working-size S2 output (ab_wls, [2][h*w][3] fp64) is upsampled with U1's arithmetic and applied to the
// ORIGINAL source with A1's, in one pass over the original pixels: BGR -> Lab, bilinear (a, b), apply, Lab -> BGR. Byte for byte the chain
// nctk_bgr2lab -> nctk_resize_f64c3 x2 -> k_apply -> nctk_lab2bgr, whose per-pixel bodies it shares (nct_pixel.h) — without the chain's original-size
// intermediates (96 B/px of fp64 coefficients and two Lab images): it reads 3 B and writes 3 B per original pixel.
//
// MI355X design: one workgroup = one 32 x 8 tile of original pixels, one thread per pixel. The working-size taps of a tile are a (32 / r + 2) x (8 / r + 2) patch
// (r = the original-to-working ratio; at most 34 x 10 since r >= 1): all 256 threads copy it to LDS once (16 KB at most, 48 B per working pixel), so a working
// pixel is fetched once per tile and not once per original pixel that it feeds. Every thread then takes its four taps per channel from LDS; at r >= 2
// neighbouring lanes read the same words (LDS broadcast). The conversion tables (23 KB) stay in global memory and are served by the vector L1 / L2 like in
// k_bgr2lab / k_lab2bgr. What binds is recorded in DESIGN.md §3.14. Its edge-aware form, the guided finish (SPEC §6.10: k_finish_guided), follows below.
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_pixel.h"

#define FU_TX 32
#define FU_TY 8
#define FU_LW (FU_TX + 2)      // a tile's taps: its first and last source index differ by at most FU_TX (scale <= 1, float rounding included), + the right / lower neighbour
#define FU_LH (FU_TY + 2)

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_up(const double* __restrict__ ab, int h, int w, const uint8_t* __restrict__ s0, int H, int W, int copy,
                                                            const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    __shared__ double tile[FU_LH * FU_LW * 6];           // [row][column][a0 a1 a2 b0 b1 b2]
    const int x0 = blockIdx.x * FU_TX, y0 = blockIdx.y * FU_TY;
    const int x1 = min(x0 + FU_TX, W) - 1, y1 = min(y0 + FU_TY, H) - 1;
    // lin_coef's source index does not decrease with the destination index: the tile's first and last pixel bound its taps
    const int sx_lo = lin_coef(x0, w, W).s, sy_lo = lin_coef(y0, h, H).s;
    const int tw = min(min(lin_coef(x1, w, W).s + 1, w - 1) - sx_lo + 1, FU_LW), th = min(min(lin_coef(y1, h, H).s + 1, h - 1) - sy_lo + 1, FU_LH);
    const size_t n3 = (size_t)h * w * 3;
    const int tid = threadIdx.y * FU_TX + threadIdx.x;
    for (int e = tid; e < tw * th * 6; e += FU_TX * FU_TY) {
        const int c6 = e % 6, p = e / 6, px = p % tw, py = p / tw;
        const size_t src = ((size_t)(sy_lo + py) * w + (sx_lo + px)) * 3;
        tile[(py * FU_LW + px) * 6 + c6] = c6 < 3 ? ab[src + c6] : ab[n3 + src + (c6 - 3)];
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = ((size_t)y * W + x) * 3;
    unsigned char lab[3];
    bgr2lab_px(s0[i], s0[i + 1], s0[i + 2], t, lab[0], lab[1], lab[2]);
    const LinCoef cx = lin_coef(x, w, W), cy = lin_coef(y, h, H);
    const int lx0 = cx.s - sx_lo, lx1 = min(cx.s + 1, w - 1) - sx_lo, ly0 = cy.s - sy_lo, ly1 = min(cy.s + 1, h - 1) - sy_lo;
    const double* p00 = tile + (ly0 * FU_LW + lx0) * 6; const double* p01 = tile + (ly0 * FU_LW + lx1) * 6;
    const double* p10 = tile + (ly1 * FU_LW + lx0) * 6; const double* p11 = tile + (ly1 * FU_LW + lx1) * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // equal sizes: U1 is a copy (nctk_resize_f64c3), not an interpolation with weights 1 and 0
        const double a = copy ? p00[c] : resize_f64_px(p00[c], p01[c], p10[c], p11[c], cx, cy);
        const double b = copy ? p00[3 + c] : resize_f64_px(p00[3 + c], p01[3 + c], p10[3 + c], p11[3 + c], cx, cy);
        lab[c] = apply_px(a, b, lab[c]);
    }
    lab2bgr_px<FORM>(lab[0], lab[1], lab[2], t, out + i);
}

int nctk_finish_upsample(nct_ctx* ctx, hipStream_t s, const double* ab_wls, int h, int w, const uint8_t* s_bgr_full, int H, int W, int form, uint8_t* out_bgr_full) {
    NCT_REQUIRE(ab_wls && s_bgr_full && out_bgr_full, "color_finish_upsample: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= NCT_FINISH_MAX_SIDE && w <= NCT_FINISH_MAX_SIDE && (long long)h * w <= NCT_FINISH_MAX_PIXELS,
                "color_finish_upsample: grid %dx%d outside [1x1, %d per side, %lld px]", w, h, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(H >= h && W >= w, "color_finish_upsample: target %dx%d smaller than the grid %dx%d", W, H, w, h);
    NCT_REQUIRE(H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS,
                "color_finish_upsample: target %dx%d above %d per side or %lld pixels", W, H, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    const void* t; NCT_TRY(nctk_cvt_tables(ctx, &t));
    const dim3 grid(cdiv(W, FU_TX), cdiv(H, FU_TY)), block(FU_TX, FU_TY);
    const int copy = (H == h && W == w) ? 1 : 0;
    if (form == 1) hipLaunchKernelGGL(k_finish_up<1>, grid, block, 0, s, ab_wls, h, w, s_bgr_full, H, W, copy, (const CvtTables*)t, out_bgr_full);
    else hipLaunchKernelGGL(k_finish_up<0>, grid, block, 0, s, ab_wls, h, w, s_bgr_full, H, W, copy, (const CvtTables*)t, out_bgr_full);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ================================================================= the guided finish (SPEC §6.10): joint-bilateral upsampling of ab_wls
// The same pass with an edge-aware stretch: every original pixel takes its (a, b) from the 4 x 4 working-size taps around lin_coef's source index, each weighted by a
// tent of half-width 2 working pixels and by how well the tap's Lab colour (the working-size source, 8 bit) matches the pixel's own: g = v u / (1 + d2 / sigma^2).
// Same workgroup shape as k_finish_up. A tile's taps run from its first pixel's s - 1 to its last pixel's s + 2, clamped to the grid. The bound: lin_coef's source index
// does not decrease with the destination index (a non-decreasing real function, rounded to float and floored, both monotone), so a thread's s lies between the tile's
// first and last; and the last exceeds the first by at most FU_TX: the real positions differ by (FU_TX - 1) * scale <= FU_TX - 1, the two float roundings (half an ulp of
// a value below 2^14: 2^-11 each) add less than 1, and floor of a difference below FU_TX adds at most FU_TX. The largest extent, FU_TX + 1 + 3, is reached at a ratio barely
// above 1 (scale just below 1 and the rounding). Hence FG_LW = FU_TX + 4 = 36 and FG_LH = FU_TY + 4 = 12.
// LDS: the six coefficient planes apart ([6][12 * 36] doubles, 20736 B: lanes of a row read consecutive doubles at ratio 1, the same double — a broadcast — at ratio
// >= 2) and the taps' Lab triples one word each in an array of their own (1728 B), 22464 B together. The 4 x 4 loop is unrolled; a skipped tap is a branch, not a
// weight of 0, so a NaN coefficient behind a zero weight stays out. What binds is recorded in DESIGN.md §3.15.
#define FG_LW (FU_TX + 4)
#define FG_LH (FU_TY + 4)

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_guided(const double* __restrict__ ab, const uint8_t* __restrict__ labw, int h, int w, const uint8_t* __restrict__ s0,
                                                                int H, int W, double s2, const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    __shared__ double tile[6][FG_LH * FG_LW];            // [a0 a1 a2 b0 b1 b2][row][column]
    __shared__ uint32_t guide[FG_LH * FG_LW];            // L | a << 8 | b << 16 of the working-size source
    const int x0 = blockIdx.x * FU_TX, y0 = blockIdx.y * FU_TY;
    const int x1 = min(x0 + FU_TX, W) - 1, y1 = min(y0 + FU_TY, H) - 1;
    const int sx_lo = max(lin_coef(x0, w, W).s - 1, 0), sy_lo = max(lin_coef(y0, h, H).s - 1, 0);
    const int tw = min(min(lin_coef(x1, w, W).s + 2, w - 1) - sx_lo + 1, FG_LW), th = min(min(lin_coef(y1, h, H).s + 2, h - 1) - sy_lo + 1, FG_LH);
    const size_t n3 = (size_t)h * w * 3;
    const int tid = threadIdx.y * FU_TX + threadIdx.x;
    for (int p = tid; p < tw * th; p += FU_TX * FU_TY) {
        const int py = p / tw, px = p - py * tw, l = py * FG_LW + px;
        const size_t src = ((size_t)(sy_lo + py) * w + (sx_lo + px)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { tile[c][l] = ab[src + c]; tile[3 + c][l] = ab[n3 + src + c]; }
        guide[l] = (uint32_t)labw[src] | ((uint32_t)labw[src + 1] << 8) | ((uint32_t)labw[src + 2] << 16);
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = ((size_t)y * W + x) * 3;
    unsigned char lab[3];
    bgr2lab_px(s0[i], s0[i + 1], s0[i + 2], t, lab[0], lab[1], lab[2]);
    const LinCoef cx = lin_coef(x, w, W), cy = lin_coef(y, h, H);
    const double fx = (double)cx.a1, fy = (double)cy.a1;
    const int lb = (cy.s - sy_lo) * FG_LW + (cx.s - sx_lo);     // the tap (0, 0); a tap inside the grid is inside the tile (the bound above)
    double den = 0.0, na[3] = {0.0, 0.0, 0.0}, nb[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = -1; j <= 2; ++j) {
        const double v = tent2_px(fy, j);
        if (cy.s + j < 0 || cy.s + j >= h || v == 0.0) continue;
#pragma unroll
        for (int k = -1; k <= 2; ++k) {
            const double u = tent2_px(fx, k);
            if (cx.s + k < 0 || cx.s + k >= w || u == 0.0) continue;
            const int l = lb + j * FG_LW + k;
            const double g = guided_weight_px(v * u, lab_d2_px(lab, guide[l]), s2);
            den += g;
#pragma unroll
            for (int c = 0; c < 3; ++c) { na[c] += g * tile[c][l]; nb[c] += g * tile[3 + c][l]; }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lab[c] = apply_px(na[c] / den, nb[c] / den, lab[c]);
    lab2bgr_px<FORM>(lab[0], lab[1], lab[2], t, out + i);
}

int nctk_finish_guided(nct_ctx* ctx, hipStream_t s, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, int H, int W, double sigma, int form,
                       uint8_t* out_bgr_full) {
    NCT_REQUIRE(ab_wls && lab_work && s_bgr_full && out_bgr_full, "color_finish_guided: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= NCT_FINISH_MAX_SIDE && w <= NCT_FINISH_MAX_SIDE && (long long)h * w <= NCT_FINISH_MAX_PIXELS,
                "color_finish_guided: grid %dx%d outside [1x1, %d per side, %lld px]", w, h, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(H >= h && W >= w, "color_finish_guided: target %dx%d smaller than the grid %dx%d", W, H, w, h);
    NCT_REQUIRE(H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS,
                "color_finish_guided: target %dx%d above %d per side or %lld pixels", W, H, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(nct_guided_sigma_ok(sigma), "color_finish_guided: sigma must be finite and > 0, and so must its square (got %g)", sigma);
    if (H == h && W == w) return nctk_finish_upsample(ctx, s, ab_wls, h, w, s_bgr_full, H, W, form, out_bgr_full);     // equal sizes: the copy path, byte for byte
    const void* t; NCT_TRY(nctk_cvt_tables(ctx, &t));
    const dim3 grid(cdiv(W, FU_TX), cdiv(H, FU_TY)), block(FU_TX, FU_TY);
    const double s2 = sigma * sigma;
    if (form == 1) hipLaunchKernelGGL(k_finish_guided<1>, grid, block, 0, s, ab_wls, lab_work, h, w, s_bgr_full, H, W, s2, (const CvtTables*)t, out_bgr_full);
    else hipLaunchKernelGGL(k_finish_guided<0>, grid, block, 0, s, ab_wls, lab_work, h, w, s_bgr_full, H, W, s2, (const CvtTables*)t, out_bgr_full);
    NCT_LAUNCH_CHECK();
    return 0;
}
