// k_finish_up_region.hip — the masked upsampling finish (SPEC §6.13 rule 4): the upsampling finish (SPEC §6.8) and its guided form (SPEC §6.10) with the compose of
// SPEC §6.11 rule 3 in the place of their Lab -> BGR, per original pixel: out = keep ? S0 : Lab2BGR(Lab_o), keep = (protect and M0 == 0) or (M0 != 255 and
// Lab_o == Lab_S on all three bytes). Byte for byte the chain nctk_finish_upsample / nctk_finish_guided up to apply_px -> k_region_compose, whose per-pixel
// bodies it shares (nct_pixel.h) — without an original-size Lab intermediate and without a second launch: it reads 3 + 1 B and writes 3 B per original pixel.
//
// MI355X design: the shape of k_finish_up.hip. One workgroup = one 32 x 8 tile of original pixels, one thread per pixel; the tile's working-size taps are staged in
// LDS once (16 KB plain, 22.5 KB guided; the bounds on their extent are derived in k_finish_up.hip and restated by the FU_ / FG_ constants here). The mask byte is one
// global read per pixel: the 32 lanes of a tile row read 32 consecutive bytes. A kept pixel stores the three source bytes its thread already holds and skips the
// cube / spline of Lab -> BGR; the branch is per lane, so a wavefront pays for the conversion as soon as one of its 64 pixels is recoloured.
// The staging loops are the ones of k_finish_up.hip, as __device__ helpers of this file: that file's device code stays what it was.
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_pixel.h"

#define FU_TX 32
#define FU_TY 8
#define FU_LW (FU_TX + 2)
#define FU_LH (FU_TY + 2)
#define FG_LW (FU_TX + 4)
#define FG_LH (FU_TY + 4)

// SPEC §6.11 rule 3 on one pixel: s = the pixel's three source bytes, lab_s / lab_o its Lab before and after A1
template <int FORM>
__device__ __forceinline__ void compose_store_px(const unsigned char* s, const unsigned char* lab_s, const unsigned char* lab_o, int M, int protect,
                                                 const CvtTables* __restrict__ t, unsigned char* __restrict__ out) {
    const bool same = lab_o[0] == lab_s[0] && lab_o[1] == lab_s[1] && lab_o[2] == lab_s[2];
    if ((protect && M == 0) || (M != 255 && same)) { out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; return; }
    lab2bgr_px<FORM>(lab_o[0], lab_o[1], lab_o[2], t, out);
}

// the plain finish's taps of the tile at (x0, y0) into tile [FU_LH][FU_LW][a0 a1 a2 b0 b1 b2]; -> the first source column and row through sx_lo / sy_lo
__device__ __forceinline__ void stage_taps_plain(const double* __restrict__ ab, int h, int w, int H, int W, int x0, int y0, int tid, double* tile, int& sx_lo, int& sy_lo) {
    const int x1 = min(x0 + FU_TX, W) - 1, y1 = min(y0 + FU_TY, H) - 1;
    sx_lo = lin_coef(x0, w, W).s; sy_lo = lin_coef(y0, h, H).s;
    const int tw = min(min(lin_coef(x1, w, W).s + 1, w - 1) - sx_lo + 1, FU_LW), th = min(min(lin_coef(y1, h, H).s + 1, h - 1) - sy_lo + 1, FU_LH);
    const size_t n3 = (size_t)h * w * 3;
    for (int e = tid; e < tw * th * 6; e += FU_TX * FU_TY) {
        const int c6 = e % 6, p = e / 6, px = p % tw, py = p / tw;
        const size_t src = ((size_t)(sy_lo + py) * w + (sx_lo + px)) * 3;
        tile[(py * FU_LW + px) * 6 + c6] = c6 < 3 ? ab[src + c6] : ab[n3 + src + (c6 - 3)];
    }
}

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_up_region(const double* __restrict__ ab, int h, int w, const uint8_t* __restrict__ s0, const uint8_t* __restrict__ mask,
                                                                   int H, int W, int copy, int protect, const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    __shared__ double tile[FU_LH * FU_LW * 6];
    const int x0 = blockIdx.x * FU_TX, y0 = blockIdx.y * FU_TY;
    int sx_lo, sy_lo;
    stage_taps_plain(ab, h, w, H, W, x0, y0, threadIdx.y * FU_TX + threadIdx.x, tile, sx_lo, sy_lo);
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x, i = p * 3;
    const int M = mask[p];
    const unsigned char s[3] = {s0[i], s0[i + 1], s0[i + 2]};
    unsigned char lab_s[3], lab[3];
    bgr2lab_px(s[0], s[1], s[2], t, lab_s[0], lab_s[1], lab_s[2]);
    const LinCoef cx = lin_coef(x, w, W), cy = lin_coef(y, h, H);
    const int lx0 = cx.s - sx_lo, lx1 = min(cx.s + 1, w - 1) - sx_lo, ly0 = cy.s - sy_lo, ly1 = min(cy.s + 1, h - 1) - sy_lo;
    const double* p00 = tile + (ly0 * FU_LW + lx0) * 6; const double* p01 = tile + (ly0 * FU_LW + lx1) * 6;
    const double* p10 = tile + (ly1 * FU_LW + lx0) * 6; const double* p11 = tile + (ly1 * FU_LW + lx1) * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a = copy ? p00[c] : resize_f64_px(p00[c], p01[c], p10[c], p11[c], cx, cy);
        const double b = copy ? p00[3 + c] : resize_f64_px(p00[3 + c], p01[3 + c], p10[3 + c], p11[3 + c], cx, cy);
        lab[c] = apply_px(a, b, lab_s[c]);
    }
    compose_store_px<FORM>(s, lab_s, lab, M, protect, t, out + i);
}

// the launchers' common checks (`who` names the entry point): those of nctk_finish_upsample / nctk_finish_guided, and the mask
static int finish_region_check(nct_ctx* ctx, const char* who, const void* ab_wls, const void* s_bgr_full, const void* mask, const void* out, int h, int w, int H, int W, int protect) {
    NCT_REQUIRE(ab_wls && s_bgr_full && out, "%s: null pointer", who);
    NCT_REQUIRE(mask, "%s: null mask", who);
    NCT_REQUIRE(protect == 0 || protect == 1, "%s: region protect must be 0 or 1 (got %d)", who, protect);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= NCT_FINISH_MAX_SIDE && w <= NCT_FINISH_MAX_SIDE && (long long)h * w <= NCT_FINISH_MAX_PIXELS,
                "%s: grid %dx%d outside [1x1, %d per side, %lld px]", who, w, h, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(H >= h && W >= w, "%s: target %dx%d smaller than the grid %dx%d", who, W, H, w, h);
    NCT_REQUIRE(H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS,
                "%s: target %dx%d above %d per side or %lld pixels", who, W, H, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    return 0;
}

int nctk_finish_upsample_region(nct_ctx* ctx, hipStream_t s, const double* ab_wls, int h, int w, const uint8_t* s_bgr_full, const uint8_t* mask, int H, int W, int protect, int form,
                                uint8_t* out_bgr_full) {
    NCT_TRY(finish_region_check(ctx, "color_finish_upsample_region", ab_wls, s_bgr_full, mask, out_bgr_full, h, w, H, W, protect));
    const void* t; NCT_TRY(nctk_cvt_tables(ctx, &t));
    const dim3 grid(cdiv(W, FU_TX), cdiv(H, FU_TY)), block(FU_TX, FU_TY);
    const int copy = (H == h && W == w) ? 1 : 0;
    if (form == 1) hipLaunchKernelGGL(k_finish_up_region<1>, grid, block, 0, s, ab_wls, h, w, s_bgr_full, mask, H, W, copy, protect, (const CvtTables*)t, out_bgr_full);
    else hipLaunchKernelGGL(k_finish_up_region<0>, grid, block, 0, s, ab_wls, h, w, s_bgr_full, mask, H, W, copy, protect, (const CvtTables*)t, out_bgr_full);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ================================================================= the masked guided finish (SPEC §6.10 rules 1-8 up to apply_px, then the compose)
// the guided finish's taps of the tile at (x0, y0): the six coefficient planes apart and the taps' Lab triples one word each, as k_finish_guided stages them
__device__ __forceinline__ void stage_taps_guided(const double* __restrict__ ab, const uint8_t* __restrict__ labw, int h, int w, int H, int W, int x0, int y0, int tid,
                                                  double (*tile)[FG_LH * FG_LW], uint32_t* guide, int& sx_lo, int& sy_lo) {
    const int x1 = min(x0 + FU_TX, W) - 1, y1 = min(y0 + FU_TY, H) - 1;
    sx_lo = max(lin_coef(x0, w, W).s - 1, 0); sy_lo = max(lin_coef(y0, h, H).s - 1, 0);
    const int tw = min(min(lin_coef(x1, w, W).s + 2, w - 1) - sx_lo + 1, FG_LW), th = min(min(lin_coef(y1, h, H).s + 2, h - 1) - sy_lo + 1, FG_LH);
    const size_t n3 = (size_t)h * w * 3;
    for (int p = tid; p < tw * th; p += FU_TX * FU_TY) {
        const int py = p / tw, px = p - py * tw, l = py * FG_LW + px;
        const size_t src = ((size_t)(sy_lo + py) * w + (sx_lo + px)) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) { tile[c][l] = ab[src + c]; tile[3 + c][l] = ab[n3 + src + c]; }
        guide[l] = (uint32_t)labw[src] | ((uint32_t)labw[src + 1] << 8) | ((uint32_t)labw[src + 2] << 16);
    }
}

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_guided_region(const double* __restrict__ ab, const uint8_t* __restrict__ labw, int h, int w, const uint8_t* __restrict__ s0,
                                                                       const uint8_t* __restrict__ mask, int H, int W, double s2, int protect, const CvtTables* __restrict__ t,
                                                                       uint8_t* __restrict__ out) {
    __shared__ double tile[6][FG_LH * FG_LW];
    __shared__ uint32_t guide[FG_LH * FG_LW];
    const int x0 = blockIdx.x * FU_TX, y0 = blockIdx.y * FU_TY;
    int sx_lo, sy_lo;
    stage_taps_guided(ab, labw, h, w, H, W, x0, y0, threadIdx.y * FU_TX + threadIdx.x, tile, guide, sx_lo, sy_lo);
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x, i = p * 3;
    const int M = mask[p];
    const unsigned char s[3] = {s0[i], s0[i + 1], s0[i + 2]};
    unsigned char lab_s[3], lab[3];
    bgr2lab_px(s[0], s[1], s[2], t, lab_s[0], lab_s[1], lab_s[2]);
    const LinCoef cx = lin_coef(x, w, W), cy = lin_coef(y, h, H);
    const double fx = (double)cx.a1, fy = (double)cy.a1;
    const int lb = (cy.s - sy_lo) * FG_LW + (cx.s - sx_lo);
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
            const double g = guided_weight_px(v * u, lab_d2_px(lab_s, guide[l]), s2);
            den += g;
#pragma unroll
            for (int c = 0; c < 3; ++c) { na[c] += g * tile[c][l]; nb[c] += g * tile[3 + c][l]; }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lab[c] = apply_px(na[c] / den, nb[c] / den, lab_s[c]);
    compose_store_px<FORM>(s, lab_s, lab, M, protect, t, out + i);
}

int nctk_finish_guided_region(nct_ctx* ctx, hipStream_t s, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, const uint8_t* mask, int H, int W,
                              double sigma, int protect, int form, uint8_t* out_bgr_full) {
    NCT_REQUIRE(lab_work, "color_finish_guided_region: null pointer");
    NCT_TRY(finish_region_check(ctx, "color_finish_guided_region", ab_wls, s_bgr_full, mask, out_bgr_full, h, w, H, W, protect));
    NCT_REQUIRE(nct_guided_sigma_ok(sigma), "color_finish_guided_region: sigma must be finite and > 0, and so must its square (got %g)", sigma);
    if (H == h && W == w) return nctk_finish_upsample_region(ctx, s, ab_wls, h, w, s_bgr_full, mask, H, W, protect, form, out_bgr_full);     // equal sizes: the copy path, byte for byte
    const void* t; NCT_TRY(nctk_cvt_tables(ctx, &t));
    const dim3 grid(cdiv(W, FU_TX), cdiv(H, FU_TY)), block(FU_TX, FU_TY);
    const double s2 = sigma * sigma;
    if (form == 1) hipLaunchKernelGGL(k_finish_guided_region<1>, grid, block, 0, s, ab_wls, lab_work, h, w, s_bgr_full, mask, H, W, s2, protect, (const CvtTables*)t, out_bgr_full);
    else hipLaunchKernelGGL(k_finish_guided_region<0>, grid, block, 0, s, ab_wls, lab_work, h, w, s_bgr_full, mask, H, W, s2, protect, (const CvtTables*)t, out_bgr_full);
    NCT_LAUNCH_CHECK();
    return 0;
}
