// k_finish_up.hip — the upsampling finish (SPEC §6.8): the working-size S2 output (ab_wls, [2][h*w][3] fp64) is upsampled with U1's arithmetic and applied to the
// ORIGINAL source with A1's, in one pass over the original pixels: BGR -> Lab, bilinear (a, b), apply, Lab -> BGR. Byte for byte the chain
// nctk_bgr2lab -> nctk_resize_f64c3 x2 -> k_apply -> nctk_lab2bgr, whose per-pixel bodies it shares (nct_pixel.h) — without the chain's original-size
// intermediates (96 B/px of fp64 coefficients and two Lab images): it reads 3 B and writes 3 B per original pixel. Four forms of one pass: plain or guided
// (SPEC §6.10: joint-bilateral weights in the place of the bilinear ones), each with or without a region mask (SPEC §6.13 rule 4: the compose of SPEC §6.11 rule 3
// in the place of the Lab -> BGR, + 1 B read per original pixel; byte for byte the chain up to apply_px -> k_region_compose, without its second launch).
//
// MI355X design: one workgroup = one 32 x 8 tile of original pixels, one thread per pixel. The working-size taps of a tile are a (32 / r + 2) x (8 / r + 2) patch
// (r = the original-to-working ratio; at most 34 x 10 since r >= 1): all 256 threads copy it to LDS once (16 KB at most, 48 B per working pixel), so a working
// pixel is fetched once per tile and not once per original pixel that it feeds. Every thread then takes its four taps per channel from LDS; at r >= 2
// neighbouring lanes read the same words (LDS broadcast). The conversion tables (23 KB) stay in global memory and are served by the vector L1 / L2 like in
// k_bgr2lab / k_lab2bgr. The mask byte is one global read per pixel: the 32 lanes of a tile row read 32 consecutive bytes. What binds is recorded in DESIGN.md
// §3.14 (plain), §3.15 (guided) and §3.18 (masked).
//
// The tiles' extents. A tile's taps run from its first pixel's source index s (guided: s - 1) to its last pixel's s + 1 (guided: s + 2), clamped to the grid. The
// bound: lin_coef's source index does not decrease with the destination index (a non-decreasing real function, rounded to float and floored, both monotone), so a
// thread's s lies between the tile's first and last; and the last exceeds the first by at most FU_TX: the real positions differ by (FU_TX - 1) * scale <= FU_TX - 1,
// the two float roundings (half an ulp of a value below 2^14: 2^-11 each) add less than 1, and floor of a difference below FU_TX adds at most FU_TX. The largest
// extent, FU_TX + 1 + 1 (guided: + 3), is reached at a ratio barely above 1 (scale just below 1 and the rounding). Hence FU_LW = FU_TX + 2 and FG_LW = FU_TX + 4.
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_pixel.h"

#define FU_TX 32
#define FU_TY 8
#define FU_LW (FU_TX + 2)
#define FU_LH (FU_TY + 2)
#define FG_LW (FU_TX + 4)
#define FG_LH (FU_TY + 4)

// where a pass ends. s = the pixel's three source bytes, lab_s / lab_o its Lab before and after A1. MASKED: SPEC §6.11 rule 3 — a kept pixel stores the source bytes
// its thread already holds and skips the cube / spline of Lab -> BGR; the branch is per lane, so a wavefront pays for the conversion as soon as one of its 64 pixels
// is recoloured. Unmasked: the conversion alone; s, lab_s and M are dead there
template <int FORM, bool MASKED>
__device__ __forceinline__ void finish_store_px(const unsigned char* s, const unsigned char* lab_s, const unsigned char* lab_o, int M, int protect,
                                                const CvtTables* __restrict__ t, unsigned char* __restrict__ out) {
    if (MASKED) {
        const bool same = lab_o[0] == lab_s[0] && lab_o[1] == lab_s[1] && lab_o[2] == lab_s[2];
        if ((protect && M == 0) || (M != 255 && same)) { out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; return; }
    }
    lab2bgr_px<FORM>(lab_o[0], lab_o[1], lab_o[2], t, out);
}

// the plain pass (mask and protect are read only if MASKED)
template <int FORM, bool MASKED>
__device__ __forceinline__ void finish_up_px(const double* __restrict__ ab, int h, int w, const uint8_t* __restrict__ s0, const uint8_t* __restrict__ mask, int H, int W, int copy,
                                             int protect, const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    __shared__ double tile[FU_LH * FU_LW * 6];           // [row][column][a0 a1 a2 b0 b1 b2]
    const int x0 = blockIdx.x * FU_TX, y0 = blockIdx.y * FU_TY;
    const int x1 = min(x0 + FU_TX, W) - 1, y1 = min(y0 + FU_TY, H) - 1;
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
    const size_t p = (size_t)y * W + x, i = p * 3;
    const int M = MASKED ? mask[p] : 255;
    const unsigned char s[3] = {s0[i], s0[i + 1], s0[i + 2]};
    unsigned char lab_s[3], lab[3];
    bgr2lab_px(s[0], s[1], s[2], t, lab_s[0], lab_s[1], lab_s[2]);
    const LinCoef cx = lin_coef(x, w, W), cy = lin_coef(y, h, H);
    const int lx0 = cx.s - sx_lo, lx1 = min(cx.s + 1, w - 1) - sx_lo, ly0 = cy.s - sy_lo, ly1 = min(cy.s + 1, h - 1) - sy_lo;
    const double* p00 = tile + (ly0 * FU_LW + lx0) * 6; const double* p01 = tile + (ly0 * FU_LW + lx1) * 6;
    const double* p10 = tile + (ly1 * FU_LW + lx0) * 6; const double* p11 = tile + (ly1 * FU_LW + lx1) * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // equal sizes: U1 is a copy (nctk_resize_f64c3), not an interpolation with weights 1 and 0
        const double a = copy ? p00[c] : resize_f64_px(p00[c], p01[c], p10[c], p11[c], cx, cy);
        const double b = copy ? p00[3 + c] : resize_f64_px(p00[3 + c], p01[3 + c], p10[3 + c], p11[3 + c], cx, cy);
        lab[c] = apply_px(a, b, lab_s[c]);
    }
    finish_store_px<FORM, MASKED>(s, lab_s, lab, M, protect, t, out + i);
}

// the guided pass (SPEC §6.10): every original pixel takes its (a, b) from the 4 x 4 working-size taps around lin_coef's source index, each weighted by a tent of
// half-width 2 working pixels and by how well the tap's Lab colour (labw: the working-size source, 8 bit) matches the pixel's own: g = v u / (1 + d2 / sigma^2).
// LDS: the six coefficient planes apart ([6][12 * 36] doubles, 20736 B: lanes of a row read consecutive doubles at ratio 1, the same double — a broadcast — at ratio
// >= 2) and the taps' Lab triples one word each in an array of their own (1728 B), 22464 B together. The 4 x 4 loop is unrolled; a skipped tap is a branch, not a
// weight of 0, so a NaN coefficient behind a zero weight stays out.
// A macro over the kernels' parameter names (ab, labw, h, w, s0, H, W, s2, t, out) and FORM, not a function like finish_up_px: the compiler simplifies a function
// before it inlines it and the kernel again afterwards, and the second pass, which meets the 16 taps unrolled, orders their operands another way — the same
// arithmetic in a schedule of 2 - 3 VGPRs more (profiles/finish_up_fold_ab.md). Expanded in the kernel the text is compiled once, as it was when each kernel spelt it
// out: the unmasked kernels are instruction for instruction what they were. mask_ and protect_ are read only if MASKED_.
#define FINISH_GUIDED_PASS(MASKED_, mask_, protect_) \
    __shared__ double tile[6][FG_LH * FG_LW];  /* [a0 a1 a2 b0 b1 b2][row][column] */                                                                 \
    __shared__ uint32_t guide[FG_LH * FG_LW];  /* L | a << 8 | b << 16 of the working-size source */                                                  \
    const int x0 = blockIdx.x * FU_TX, y0 = blockIdx.y * FU_TY;                                                                                       \
    const int x1 = min(x0 + FU_TX, W) - 1, y1 = min(y0 + FU_TY, H) - 1;                                                                               \
    const int sx_lo = max(lin_coef(x0, w, W).s - 1, 0), sy_lo = max(lin_coef(y0, h, H).s - 1, 0);                                                     \
    const int tw = min(min(lin_coef(x1, w, W).s + 2, w - 1) - sx_lo + 1, FG_LW), th = min(min(lin_coef(y1, h, H).s + 2, h - 1) - sy_lo + 1, FG_LH);   \
    const size_t n3 = (size_t)h * w * 3;                                                                                                              \
    const int tid = threadIdx.y * FU_TX + threadIdx.x;                                                                                                \
    for (int p = tid; p < tw * th; p += FU_TX * FU_TY) {                                                                                              \
        const int py = p / tw, px = p - py * tw, l = py * FG_LW + px;                                                                                 \
        const size_t src = ((size_t)(sy_lo + py) * w + (sx_lo + px)) * 3;                                                                             \
_Pragma("unroll")                                                                                                                                     \
        for (int c = 0; c < 3; ++c) { tile[c][l] = ab[src + c]; tile[3 + c][l] = ab[n3 + src + c]; }                                                  \
        guide[l] = (uint32_t)labw[src] | ((uint32_t)labw[src + 1] << 8) | ((uint32_t)labw[src + 2] << 16);                                            \
    }                                                                                                                                                 \
    __syncthreads();                                                                                                                                  \
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;                                                                                             \
    if (x >= W || y >= H) return;                                                                                                                     \
    const size_t p = (size_t)y * W + x, i = p * 3;                                                                                                    \
    const int M = MASKED_ ? (mask_)[p] : 255;                                                                                                         \
    const unsigned char s[3] = {s0[i], s0[i + 1], s0[i + 2]};                                                                                         \
    unsigned char lab_s[3], lab[3];                                                                                                                   \
    bgr2lab_px(s[0], s[1], s[2], t, lab_s[0], lab_s[1], lab_s[2]);                                                                                    \
    const LinCoef cx = lin_coef(x, w, W), cy = lin_coef(y, h, H);                                                                                     \
    const double fx = (double)cx.a1, fy = (double)cy.a1;                                                                                              \
    const int lb = (cy.s - sy_lo) * FG_LW + (cx.s - sx_lo);  /* the tap (0, 0); a tap inside the grid is inside the tile (the bound above) */         \
    double den = 0.0, na[3] = {0.0, 0.0, 0.0}, nb[3] = {0.0, 0.0, 0.0};                                                                               \
_Pragma("unroll")                                                                                                                                     \
    for (int j = -1; j <= 2; ++j) {                                                                                                                   \
        const double v = tent2_px(fy, j);                                                                                                             \
        if (cy.s + j < 0 || cy.s + j >= h || v == 0.0) continue;                                                                                      \
_Pragma("unroll")                                                                                                                                     \
        for (int k = -1; k <= 2; ++k) {                                                                                                               \
            const double u = tent2_px(fx, k);                                                                                                         \
            if (cx.s + k < 0 || cx.s + k >= w || u == 0.0) continue;                                                                                  \
            const int l = lb + j * FG_LW + k;                                                                                                         \
            const double g = guided_weight_px(v * u, lab_d2_px(lab_s, guide[l]), s2);                                                                 \
            den += g;                                                                                                                                 \
_Pragma("unroll")                                                                                                                                     \
            for (int c = 0; c < 3; ++c) { na[c] += g * tile[c][l]; nb[c] += g * tile[3 + c][l]; }                                                     \
        }                                                                                                                                             \
    }                                                                                                                                                 \
_Pragma("unroll")                                                                                                                                     \
    for (int c = 0; c < 3; ++c) lab[c] = apply_px(na[c] / den, nb[c] / den, lab_s[c]);                                                                \
    finish_store_px<FORM, MASKED_>(s, lab_s, lab, M, (protect_), t, out + i);

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_up(const double* __restrict__ ab, int h, int w, const uint8_t* __restrict__ s0, int H, int W, int copy,
                                                            const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    finish_up_px<FORM, false>(ab, h, w, s0, nullptr, H, W, copy, 0, t, out);
}

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_up_region(const double* __restrict__ ab, int h, int w, const uint8_t* __restrict__ s0, const uint8_t* __restrict__ mask,
                                                                   int H, int W, int copy, int protect, const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    finish_up_px<FORM, true>(ab, h, w, s0, mask, H, W, copy, protect, t, out);
}

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_guided(const double* __restrict__ ab, const uint8_t* __restrict__ labw, int h, int w, const uint8_t* __restrict__ s0,
                                                                int H, int W, double s2, const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    FINISH_GUIDED_PASS(false, (const uint8_t*)nullptr, 0)
}

template <int FORM>
__global__ __launch_bounds__(FU_TX * FU_TY) void k_finish_guided_region(const double* __restrict__ ab, const uint8_t* __restrict__ labw, int h, int w, const uint8_t* __restrict__ s0,
                                                                       const uint8_t* __restrict__ mask, int H, int W, double s2, int protect, const CvtTables* __restrict__ t,
                                                                       uint8_t* __restrict__ out) {
    FINISH_GUIDED_PASS(true, mask, protect)
}

int nctk_finish_up_check(nct_ctx* ctx, bool guided, const void* ab_wls, const void* lab_work, int h, int w, const nct_finish_up& up) {
    const char* who = nct_finish_up_name(guided, up.mask != nullptr);
    NCT_REQUIRE(ab_wls && (lab_work || !guided) && up.s_bgr && up.out_bgr, "%s: null pointer", who);
    NCT_REQUIRE(!up.mask || up.protect == 0 || up.protect == 1, "%s: region protect must be 0 or 1 (got %d)", who, up.protect);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= NCT_FINISH_MAX_SIDE && w <= NCT_FINISH_MAX_SIDE && (long long)h * w <= NCT_FINISH_MAX_PIXELS,
                "%s: grid %dx%d outside [1x1, %d per side, %lld px]", who, w, h, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(up.H >= h && up.W >= w, "%s: target %dx%d smaller than the grid %dx%d", who, up.W, up.H, w, h);
    NCT_REQUIRE(up.H <= NCT_FINISH_MAX_SIDE && up.W <= NCT_FINISH_MAX_SIDE && (long long)up.H * up.W <= NCT_FINISH_MAX_PIXELS,
                "%s: target %dx%d above %d per side or %lld pixels", who, up.W, up.H, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(!guided || nct_guided_sigma_ok(up.sigma), "%s: sigma must be finite and > 0, and so must its square (got %g)", who, up.sigma);
    return 0;
}

int nctk_finish_up(nct_ctx* ctx, hipStream_t s, const double* ab_wls, const uint8_t* lab_work, int h, int w, const nct_finish_up& up) {
    const bool guided = up.sigma > 0.0, cube = up.form == 1;
    NCT_TRY(nctk_finish_up_check(ctx, guided, ab_wls, lab_work, h, w, up));
    const void* tv; NCT_TRY(nctk_cvt_tables(ctx, &tv));
    const CvtTables* t = (const CvtTables*)tv;
    const dim3 grid(cdiv(up.W, FU_TX), cdiv(up.H, FU_TY)), block(FU_TX, FU_TY);
    const int H = up.H, W = up.W, copy = (H == h && W == w) ? 1 : 0;
    const double s2 = up.sigma * up.sigma;
    if (guided && !copy) {
        if (up.mask) hipLaunchKernelGGL((cube ? k_finish_guided_region<1> : k_finish_guided_region<0>), grid, block, 0, s, ab_wls, lab_work, h, w, up.s_bgr, up.mask, H, W, s2, up.protect, t, up.out_bgr);
        else hipLaunchKernelGGL((cube ? k_finish_guided<1> : k_finish_guided<0>), grid, block, 0, s, ab_wls, lab_work, h, w, up.s_bgr, H, W, s2, t, up.out_bgr);
    } else {                                             // plain, or guided at equal sizes: the copy path, byte for byte
        if (up.mask) hipLaunchKernelGGL((cube ? k_finish_up_region<1> : k_finish_up_region<0>), grid, block, 0, s, ab_wls, h, w, up.s_bgr, up.mask, H, W, copy, up.protect, t, up.out_bgr);
        else hipLaunchKernelGGL((cube ? k_finish_up<1> : k_finish_up<0>), grid, block, 0, s, ab_wls, h, w, up.s_bgr, H, W, copy, t, up.out_bgr);
    }
    NCT_LAUNCH_CHECK();
    return 0;
}
