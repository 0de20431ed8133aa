// k_cvt.hip — 8-bit BGR<->Lab conversion and bilinear resizes on the GPU (A1 + the cv::resize / cvtColor call sites).
// Reference call sites: cvtColor(BGR2Lab) main.cu:352,371, ColorTransfer.h:58; cvtColor(Lab2BGR) ColorTransfer.cpp:1469;
// resize(INTER_LINEAR) 8UC3 main.cu:106-107, 64FC3 ColorTransfer.cpp:462-463. The arithmetic is OpenCV 2.4.10's
// (external dependency, not under /root/reference): integer RGB2Lab_b with the sRGB-gamma and cube-root LUTs, float
// Lab2RGB with the cubic-spline inverse-gamma table, fixed-point (11-bit) bilinear with the >>4,*b,>>16,+2,>>2 chain and
// the silent INTER_AREA switch for exact 2x shrink.
// All kernels are trivially bandwidth bound (3-24 B per pixel).
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_pixel.h"
#include <cmath>
#include <mutex>

namespace {
inline int cv_round_h(double v) { return (int)lrint(v); }
inline unsigned short sat_u16(float v) { int i = cv_round_h(v); return (unsigned short)(i < 0 ? 0 : (i > 65535 ? 65535 : i)); }

void build_tables(CvtTables& t) {
    for (int i = 0; i < 256; i++) {
        float x = i * (1.f / 255.f);
        t.gamma[i] = sat_u16(255.f * (1 << GAMMA_SHIFT) * (x <= 0.04045f ? x * (1.f / 12.92f) : (float)pow((double)(x + 0.055) * (1. / 1.055), 2.4)));
    }
    for (int i = 0; i < CBRT_TAB; i++) {
        float x = i * (1.f / (255.f * (1 << GAMMA_SHIFT)));
        t.cbrt[i] = sat_u16((1 << LAB_SHIFT2) * (x < 0.008856f ? x * 7.787f + 0.13793103448275862f : cbrtf(x)));
    }
    static float g[GAMMA_TAB + 1];
    for (int i = 0; i <= GAMMA_TAB; i++) {
        float x = i * (1.f / GAMMA_TAB);
        g[i] = x <= 0.0031308 ? x * 12.92f : (float)(1.055 * pow((double)x, 1. / 2.4) - 0.055);
    }
    // natural cubic spline through g (OpenCV splineBuild)
    float* tab = t.inv_gamma; const int n = GAMMA_TAB; float cn = 0;
    tab[0] = tab[1] = 0.f;
    for (int i = 1; i < n - 1; i++) {
        float tt = 3 * (g[i + 1] - 2 * g[i] + g[i - 1]);
        float l = 1 / (4 - tab[(i - 1) * 4]);
        tab[i * 4] = l; tab[i * 4 + 1] = (tt - tab[(i - 1) * 4 + 1]) * l;
    }
    for (int i = n - 1; i >= 0; i--) {
        float c = tab[i * 4 + 1] - tab[i * 4] * cn;
        float b = g[i + 1] - g[i] - (cn + c * 2) * 0.3333333333333333f;
        float d = (cn - c) * 0.3333333333333333f;
        tab[i * 4] = g[i]; tab[i * 4 + 1] = b; tab[i * 4 + 2] = c; tab[i * 4 + 3] = d;
        cn = c;
    }
    const float s2x[9] = {0.412453f, 0.357580f, 0.180423f, 0.212671f, 0.715160f, 0.072169f, 0.019334f, 0.119193f, 0.950227f};
    const float wp[3] = {0.950456f, 1.f, 1.088754f};
    const float scale[3] = {(1 << LAB_SHIFT) / wp[0], (float)(1 << LAB_SHIFT), (1 << LAB_SHIFT) / wp[2]};
    for (int i = 0; i < 3; i++) {     // BGR input: the R coefficient sits in column 2, the B coefficient in column 0
        t.coeffs[i * 3 + 2] = cv_round_h(s2x[i * 3] * scale[i]);
        t.coeffs[i * 3 + 1] = cv_round_h(s2x[i * 3 + 1] * scale[i]);
        t.coeffs[i * 3 + 0] = cv_round_h(s2x[i * 3 + 2] * scale[i]);
    }
    const float x2s[9] = {3.240479f, -1.53715f, -0.498535f, -0.969256f, 1.875991f, 0.041556f, 0.055648f, -0.204043f, 1.057311f};
    for (int i = 0; i < 3; i++) { t.l2r[i + 6] = x2s[i] * wp[i]; t.l2r[i + 3] = x2s[i + 3] * wp[i]; t.l2r[i] = x2s[i + 6] * wp[i]; }
}
}  // namespace

struct cvt_dev { CvtTables* d = nullptr; };

static int get_tables(nct_ctx* ctx, const CvtTables** out) {
    if (!ctx->cvt) {
        CvtTables* h = new CvtTables();
        build_tables(*h);
        cvt_dev* cd = new cvt_dev();
        hipError_t e = hipMalloc(&cd->d, sizeof(CvtTables));
        if (e == hipSuccess) e = hipMemcpy(cd->d, h, sizeof(CvtTables), hipMemcpyHostToDevice);
        delete h;
        if (e != hipSuccess) { delete cd; return ctx->fail(NCT_ERR_HIP, "colour tables: %s", hipGetErrorString(e)); }
        ctx->cvt = cd;
    }
    *out = ((cvt_dev*)ctx->cvt)->d;
    return 0;
}
int nctk_cvt_tables(nct_ctx* ctx, const void** out) { const CvtTables* t; NCT_TRY(get_tables(ctx, &t)); *out = t; return 0; }
void nct_cvt_free(nct_ctx* ctx) { if (ctx->cvt) { cvt_dev* cd = (cvt_dev*)ctx->cvt; if (cd->d) (void)hipFree(cd->d); delete cd; ctx->cvt = nullptr; } }

// the per-pixel bodies live in nct_pixel.h (the upsampling finish shares them)
__global__ void k_bgr2lab(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n, const CvtTables* __restrict__ t) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bgr2lab_px(src[i * 3], src[i * 3 + 1], src[i * 3 + 2], t, dst[i * 3], dst[i * 3 + 1], dst[i * 3 + 2]);
}

// CV_Lab2BGR on 8U = Lab2RGB_b: L * 100/255, a - 128, b - 128 -> float Lab2RGB_f -> * 255 -> saturate_cast<uchar> (cvRound). Two forms of Lab2RGB_f exist in
// OpenCV's history; the sources of the reference's pinned release cannot be inspected here, its result images can:
//   FORM 0 (default, NCT_LAB2BGR_PIECEWISE): CIE's linear branch for L* <= 8 and f <= 6/29, linear RGB clipped to [0, 1] before the inverse-gamma table. The
//           reference's own demo results contain (0, 0, 0) and (0, 2, 0)-like pixels, which only this form can produce (include/nct.h).
//   FORM 1 (NCT_FLAG_LAB2BGR_CUBE): the older form — fY = (L + 16) * (1/116), fX = fY + a * 0.002f, fZ = fY - b * 0.005f, every one cubed, NO clipping of the
//           linear RGB: the spline is evaluated at the clamped table index with the unclamped offset (it extrapolates its first / last cubic), only the
//           final cast saturates. Black comes out as (9, 9, 9).
// They agree wherever L* > 8, fX and fZ > 6/29 and the colour is inside the sRGB gamut. Both are pinned by independent evaluations (tests/test_oracle_color.py).
template <int FORM>
__global__ void k_lab2bgr(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t n, const CvtTables* __restrict__ t) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lab2bgr_px<FORM>(src[i * 3], src[i * 3 + 1], src[i * 3 + 2], t, dst + i * 3);
}

int nctk_bgr2lab(nct_ctx* ctx, hipStream_t s, const uint8_t* src, uint8_t* dst, size_t npix) {
    const CvtTables* t; NCT_TRY(get_tables(ctx, &t));
    hipLaunchKernelGGL(k_bgr2lab, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, src, dst, npix, t);
    NCT_LAUNCH_CHECK();
    return 0;
}
int nctk_lab2bgr(nct_ctx* ctx, hipStream_t s, const uint8_t* src, uint8_t* dst, size_t npix, int form) {
    const CvtTables* t; NCT_TRY(get_tables(ctx, &t));
    if (form == 1) hipLaunchKernelGGL(k_lab2bgr<1>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, src, dst, npix, t);
    else hipLaunchKernelGGL(k_lab2bgr<0>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, src, dst, npix, t);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- resize
__global__ void k_resize_u8c3(const uint8_t* __restrict__ src, int sh, int sw, uint8_t* __restrict__ dst, int dh, int dw, int area2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dh * dw) return;
    const int dy = i / dw, dx = i - dy * dw;
    if (area2) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint8_t* p = src + ((size_t)(2 * dy) * sw + 2 * dx) * 3 + c;
            dst[(size_t)i * 3 + c] = (uint8_t)((p[0] + p[3] + p[(size_t)sw * 3] + p[(size_t)sw * 3 + 3] + 2) >> 2);
        }
        return;
    }
    const LinCoef cx = lin_coef(dx, sw, dw), cy = lin_coef(dy, sh, dh);
    const int a0 = (short)(int)rintf(cx.a0 * 2048.f), a1 = (short)(int)rintf(cx.a1 * 2048.f);
    const int b0 = (short)(int)rintf(cy.a0 * 2048.f), b1 = (short)(int)rintf(cy.a1 * 2048.f);
    const int sy0 = cy.s, sy1 = min(cy.s + 1, sh - 1);
    const int sx1 = min(cx.s + 1, sw - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int p00 = src[((size_t)sy0 * sw + cx.s) * 3 + c], p01 = src[((size_t)sy0 * sw + sx1) * 3 + c];
        const int p10 = src[((size_t)sy1 * sw + cx.s) * 3 + c], p11 = src[((size_t)sy1 * sw + sx1) * 3 + c];
        const int r0 = cx.tail ? p00 * 2048 : p00 * a0 + p01 * a1;
        const int r1 = cx.tail ? p10 * 2048 : p10 * a0 + p11 * a1;
        dst[(size_t)i * 3 + c] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
    }
}

int nctk_resize_u8c3(nct_ctx* ctx, hipStream_t s, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw) {
    if (sh == dh && sw == dw) { NCT_HIP(hipMemcpyAsync(dst, src, (size_t)sh * sw * 3, hipMemcpyDeviceToDevice, s)); return 0; }
    const int area2 = (sw == dw * 2 && sh == dh * 2) ? 1 : 0;
    hipLaunchKernelGGL(k_resize_u8c3, dim3(cdiv(dh * dw, 256)), dim3(256), 0, s, src, sh, sw, dst, dh, dw, area2);
    NCT_LAUNCH_CHECK();
    return 0;
}

// 64FC3 bilinear (upsampling of the a,b coefficient maps): float weights, double accumulation, horizontal then vertical
__global__ void k_resize_f64c3(const double* __restrict__ src, int sh, int sw, double* __restrict__ dst, int dh, int dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dh * dw) return;
    const int dy = i / dw, dx = i - dy * dw;
    const LinCoef cx = lin_coef(dx, sw, dw), cy = lin_coef(dy, sh, dh);
    const int sy0 = cy.s, sy1 = min(cy.s + 1, sh - 1), sx1 = min(cx.s + 1, sw - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        dst[(size_t)i * 3 + c] = resize_f64_px(src[((size_t)sy0 * sw + cx.s) * 3 + c], src[((size_t)sy0 * sw + sx1) * 3 + c],
                                               src[((size_t)sy1 * sw + cx.s) * 3 + c], src[((size_t)sy1 * sw + sx1) * 3 + c], cx, cy);
}

int nctk_resize_f64c3(nct_ctx* ctx, hipStream_t s, const double* src, int sh, int sw, double* dst, int dh, int dw) {
    if (sh == dh && sw == dw) { NCT_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)sh * sw * 3, hipMemcpyDeviceToDevice, s)); return 0; }
    hipLaunchKernelGGL(k_resize_f64c3, dim3(cdiv(dh * dw, 256)), dim3(256), 0, s, src, sh, sw, dst, dh, dw);
    NCT_LAUNCH_CHECK();
    return 0;
}
