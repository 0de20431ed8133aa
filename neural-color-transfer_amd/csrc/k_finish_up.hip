// k_finish_up.hip — the upsampling finish (SPEC §6.8): the working-size S2 output (ab_wls, [2][h*w][3] fp64) is upsampled with U1's arithmetic and applied to the
// ORIGINAL source with A1's, in one pass over the original pixels: BGR -> Lab, bilinear (a, b), apply, Lab -> BGR. Byte for byte the chain
// nctk_bgr2lab -> nctk_resize_f64c3 x2 -> k_apply -> nctk_lab2bgr, whose per-pixel bodies it shares (nct_pixel.h) — without the chain's original-size
// intermediates (96 B/px of fp64 coefficients and two Lab images): it reads 3 B and writes 3 B per original pixel.
//
// MI355X design: one workgroup = one 32 x 8 tile of original pixels, one thread per pixel. The working-size taps of a tile are a (32 / r + 2) x (8 / r + 2) patch
// (r = the original-to-working ratio; at most 34 x 10 since r >= 1): all 256 threads copy it to LDS once (16 KB at most, 48 B per working pixel), so a working
// pixel is fetched once per tile and not once per original pixel that it feeds. Every thread then takes its four taps per channel from LDS; at r >= 2
// neighbouring lanes read the same words (LDS broadcast). The conversion tables (23 KB) stay in global memory and are served by the vector L1 / L2 like in
// k_bgr2lab / k_lab2bgr. What binds is recorded in DESIGN.md §3.14.
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
