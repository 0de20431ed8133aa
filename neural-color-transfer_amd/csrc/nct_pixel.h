// nct_pixel.h — the per-pixel bodies of the 8-bit BGR<->Lab conversions (k_cvt.hip), of the 64FC3 bilinear resize (k_cvt.hip) and of A1 (k_colorsolve.hip), as
// __device__ functions: the kernels that run one of them per launch and the upsampling finish (k_finish_up.hip, SPEC §6.8), which runs all four per pixel,
// share ONE copy of each expression; the guided finish (SPEC §6.10) adds its tap weights below. The build has -ffp-contract=off: an expression written once rounds the same way wherever it is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

enum { LAB_SHIFT = 12, LAB_SHIFT2 = 15, GAMMA_SHIFT = 3, CBRT_TAB = 256 * 3 / 2 * (1 << GAMMA_SHIFT), GAMMA_TAB = 1024 };

// the conversion tables on the device (built on the host by k_cvt.hip, one copy per context)
struct CvtTables { unsigned short gamma[256]; unsigned short cbrt[CBRT_TAB]; float inv_gamma[GAMMA_TAB * 4]; int coeffs[9]; float l2r[9]; };

#define DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
#define LAB_D(u) ((double)(u) * (1.0 / 255.0))      // Mat::convertTo(CV_64F, 1/255)

__device__ __forceinline__ unsigned char sat8(int v) { return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// CV_BGR2Lab on 8U = RGB2Lab_b: integer arithmetic through the sRGB-gamma and cube-root tables
__device__ __forceinline__ void bgr2lab_px(int b8, int g8, int r8, const CvtTables* __restrict__ t, unsigned char& L, unsigned char& a, unsigned char& b) {
    const int Lscale = (116 * 255 + 50) / 100;
    const int Lshift = -((16 * 255 * (1 << LAB_SHIFT2) + 50) / 100);
    const int R = t->gamma[b8], G = t->gamma[g8], B = t->gamma[r8];
    const int* C = t->coeffs;
    const int fX = t->cbrt[DESCALE(R * C[0] + G * C[1] + B * C[2], LAB_SHIFT)];
    const int fY = t->cbrt[DESCALE(R * C[3] + G * C[4] + B * C[5], LAB_SHIFT)];
    const int fZ = t->cbrt[DESCALE(R * C[6] + G * C[7] + B * C[8], LAB_SHIFT)];
    L = sat8(DESCALE(Lscale * fY + Lshift, LAB_SHIFT2));
    a = sat8(DESCALE(500 * (fX - fY) + 128 * (1 << LAB_SHIFT2), LAB_SHIFT2));
    b = sat8(DESCALE(200 * (fY - fZ) + 128 * (1 << LAB_SHIFT2), LAB_SHIFT2));
}

__device__ __forceinline__ float spline_eval(float x, const float* __restrict__ tab) {
    int ix = (int)floorf(x);
    ix = ix < 0 ? 0 : (ix > GAMMA_TAB - 1 ? GAMMA_TAB - 1 : ix);
    x -= (float)ix;
    tab += ix * 4;
    return ((tab[3] * x + tab[2]) * x + tab[1]) * x + tab[0];
}

// CV_Lab2BGR on 8U in one of its two forms (k_cvt.hip describes them): FORM 0 piecewise, FORM 1 plain cube
template <int FORM>
__device__ __forceinline__ void lab2bgr_px(int L8, int a8, int b8, const CvtTables* __restrict__ t, unsigned char* __restrict__ bgr) {
    const float li = (float)L8 * (100.f / 255.f), ai = (float)(a8 - 128), bi = (float)(b8 - 128);
    float fx, y, fz;
    if constexpr (FORM == 1) {
        const float fy = (li + 16.f) * (1.f / 116.f);
        fx = fy + ai * 0.002f; fz = fy - bi * 0.005f;
        y = fy * fy * fy; fx = fx * fx * fx; fz = fz * fz * fz;
    } else {
        const float lThresh = 0.008856f * 903.3f;
        const float fThresh = 7.787f * 0.008856f + 16.0f / 116.0f;
        float fy;
        if (li <= lThresh) { y = li / 903.3f; fy = 7.787f * y + 16.0f / 116.0f; }
        else { fy = (li + 16.0f) / 116.0f; y = fy * fy * fy; }
        fx = ai / 500.0f + fy; fz = fy - bi / 200.0f;
        fx = fx <= fThresh ? (fx - 16.0f / 116.0f) / 7.787f : fx * fx * fx;
        fz = fz <= fThresh ? (fz - 16.0f / 116.0f) / 7.787f : fz * fz * fz;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = t->l2r[k * 3] * fx + t->l2r[k * 3 + 1] * y + t->l2r[k * 3 + 2] * fz;
        if constexpr (FORM == 0) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        v = spline_eval(v * (float)GAMMA_TAB, t->inv_gamma);
        v = v * 255.f;
        // saturate_cast<uchar>(float) = saturate(cvRound(v)); the clamp in float first keeps the conversion defined for extrapolated values
        v = v < -1.f ? -1.f : (v > 256.f ? 256.f : v);
        bgr[k] = sat8((int)rintf(v));
    }
}

// cv::resize(INTER_LINEAR): source index and weights of destination index d
struct LinCoef { int s; float a0, a1; bool tail; };     // tail: dx >= xmax => D = S[s] * ONE
__device__ __forceinline__ LinCoef lin_coef(int d, int ssize, int dsize) {
    const double scale = (double)ssize / (double)dsize;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    bool tail = false;
    if (s + 1 >= ssize) { tail = true; if (s >= ssize - 1) { f = 0.f; s = ssize - 1; } }
    return LinCoef{s, 1.f - f, f, tail};
}

// 8UC1 bilinear, one destination pixel of a sh x sw image: cv::resize's 11-bit fixed-point chain (weights rounded to 1/2048, >> 4, * b, >> 16, + 2, >> 2) — the arithmetic
// of k_resize_u8c3 / k_resize_u8c1 on one byte, for kernels that resize inside another step
__device__ __forceinline__ int resize_u8_px(const unsigned char* __restrict__ src, int sh, int sw, int dy, int dx, int dh, int dw) {
    const LinCoef cx = lin_coef(dx, sw, dw), cy = lin_coef(dy, sh, dh);
    const int a0 = (short)(int)rintf(cx.a0 * 2048.f), a1 = (short)(int)rintf(cx.a1 * 2048.f);
    const int b0 = (short)(int)rintf(cy.a0 * 2048.f), b1 = (short)(int)rintf(cy.a1 * 2048.f);
    const int sy0 = cy.s, sy1 = min(cy.s + 1, sh - 1);
    const int sx1 = min(cx.s + 1, sw - 1);
    const int p00 = src[(size_t)sy0 * sw + cx.s], p01 = src[(size_t)sy0 * sw + sx1];
    const int p10 = src[(size_t)sy1 * sw + cx.s], p11 = src[(size_t)sy1 * sw + sx1];
    const int r0 = cx.tail ? p00 * 2048 : p00 * a0 + p01 * a1;
    const int r1 = cx.tail ? p10 * 2048 : p10 * a0 + p11 * a1;
    return (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
}

// 64FC3 bilinear, one channel of one destination pixel from its four taps: float weights, double accumulation, horizontal then vertical
__device__ __forceinline__ double resize_f64_px(double p00, double p01, double p10, double p11, const LinCoef& cx, const LinCoef& cy) {
    const double a0 = (double)cx.a0, a1 = (double)cx.a1, b0 = (double)cy.a0, b1 = (double)cy.a1;
    const double r0 = cx.tail ? p00 * 1.0 : p00 * a0 + p01 * a1;
    const double r1 = cx.tail ? p10 * 1.0 : p10 * a0 + p11 * a1;
    return r0 * b0 + r1 * b1;
}

// SPEC §6.10, the guided upsampling finish (k_finish_up.hip: k_finish_guided). The spatial weight of the tap at offset j (-1 .. 2) from lin_coef's source index, f its
// fraction as a double: a tent of half-width 2 working pixels; 0 only at j = 2 with f = 0
__device__ __forceinline__ double tent2_px(double f, int j) { return 1.0 - fabs(f - (double)j) * 0.5; }
// the squared distance of two Lab triples, lw packed L | a << 8 | b << 16: 0 .. 195075
__device__ __forceinline__ int lab_d2_px(const unsigned char* lab, unsigned lw) {
    const int d0 = (int)lab[0] - (int)(lw & 255u), d1 = (int)lab[1] - (int)((lw >> 8) & 255u), d2 = (int)lab[2] - (int)((lw >> 16) & 255u);
    return d0 * d0 + d1 * d1 + d2 * d2;
}
// a tap's weight: its spatial weight vu over 1 + d2 / sigma^2 (IEEE division twice, no transcendental)
__device__ __forceinline__ double guided_weight_px(double vu, int d2, double s2) { return vu / (1.0 + (double)d2 / s2); }

// A1: one Lab byte recoloured by its coefficients (ColorTransfer.cpp:1452-1466)
__device__ __forceinline__ unsigned char apply_px(double a, double b, unsigned char lab) {
    double v = LAB_D(lab) * a + b;
    v = v > 0.0 ? v : 0.0; v = v < 1.0 ? v : 1.0;
    const int q = (int)rint(v * 255.0);
    return (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
}
