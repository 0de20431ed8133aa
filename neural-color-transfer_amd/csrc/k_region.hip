// k_region.hip — source region masks (SPEC §6.11): the single-channel resize of the level masks, the mix of S1's coefficients toward the identity transform, and the
// compose of a level's result with the untouched source. tests/region_ref.py is the numpy form of every operation here.
// All three are streams, one thread per pixel, bounded by their bytes: the resize 4 B in + 1 B out per output pixel, the mix 1 + 48 B in and 48 B out per level
// pixel (nothing but the mask byte where M is 0 or, in place, 255), the compose 3 + 3 + 3 + 1 B in and 3 B out.
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_pixel.h"

// rule 1: channel 0 of k_resize_u8c3 (k_cvt.hip) on (M, M, M) — the same fixed-point bilinear chain and the same 2x area case, one byte per pixel
__global__ void k_resize_u8c1(const uint8_t* __restrict__ src, int sh, int sw, uint8_t* __restrict__ dst, int dh, int dw, int area2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dh * dw) return;
    const int dy = i / dw, dx = i - dy * dw;
    if (area2) {
        const uint8_t* p = src + (size_t)(2 * dy) * sw + 2 * dx;
        dst[i] = (uint8_t)((p[0] + p[1] + p[sw] + p[sw + 1] + 2) >> 2);
        return;
    }
    const LinCoef cx = lin_coef(dx, sw, dw), cy = lin_coef(dy, sh, dh);
    const int a0 = (short)(int)rintf(cx.a0 * 2048.f), a1 = (short)(int)rintf(cx.a1 * 2048.f);
    const int b0 = (short)(int)rintf(cy.a0 * 2048.f), b1 = (short)(int)rintf(cy.a1 * 2048.f);
    const int sy0 = cy.s, sy1 = min(cy.s + 1, sh - 1);
    const int sx1 = min(cx.s + 1, sw - 1);
    const int p00 = src[(size_t)sy0 * sw + cx.s], p01 = src[(size_t)sy0 * sw + sx1];
    const int p10 = src[(size_t)sy1 * sw + cx.s], p11 = src[(size_t)sy1 * sw + sx1];
    const int r0 = cx.tail ? p00 * 2048 : p00 * a0 + p01 * a1;
    const int r1 = cx.tail ? p10 * 2048 : p10 * a0 + p11 * a1;
    dst[i] = (uint8_t)((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
}

int nctk_resize_u8c1(nct_ctx* ctx, hipStream_t s, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw) {
    if (sh == dh && sw == dw) { NCT_HIP(hipMemcpyAsync(dst, src, (size_t)sh * sw, hipMemcpyDeviceToDevice, s)); return 0; }
    const int area2 = (sw == dw * 2 && sh == dh * 2) ? 1 : 0;
    hipLaunchKernelGGL(k_resize_u8c1, dim3(cdiv(dh * dw, 256)), dim3(256), 0, s, src, sh, sw, dst, dh, dw, area2);
    NCT_LAUNCH_CHECK();
    return 0;
}

// rule 2: per level pixel a' = 1 + m (a - 1), b' = m b with m = M / 255 in double; M = 255 copies the six words (a NaN stays that NaN), M = 0 writes the identity
// transform (a NaN is healed). x_out may be x: a thread reads its pixel before it writes it, and then an M = 255 pixel is neither read nor written
__global__ void k_region_mix(const double* x, const uint8_t* __restrict__ mask, int n, double* x_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int M = mask[i];
    const size_t ia = (size_t)3 * i, ib = (size_t)3 * n + ia;
    if (M == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { x_out[ia + c] = 1.0; x_out[ib + c] = 0.0; }
        return;
    }
    if (M == 255) {
        if (x_out == x) return;
        const unsigned long long* xi = (const unsigned long long*)x;
        unsigned long long* xo = (unsigned long long*)x_out;
#pragma unroll
        for (int c = 0; c < 3; ++c) { xo[ia + c] = xi[ia + c]; xo[ib + c] = xi[ib + c]; }
        return;
    }
    const double m = (double)M / 255.0;
    double a[3], b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = x[ia + c]; b[c] = x[ib + c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { x_out[ia + c] = 1.0 + m * (a[c] - 1.0); x_out[ib + c] = m * b[c]; }
}

int nctk_region_mix(nct_ctx* ctx, hipStream_t s, const double* x, const uint8_t* mask, int h, int w, double* x_out) {
    NCT_REQUIRE(x && mask && x_out, "region_mix: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "region_mix: grid %dx%d out of range", w, h);
    const int n = h * w;
    hipLaunchKernelGGL(k_region_mix, dim3(cdiv(n, 256)), dim3(256), 0, s, x, mask, n, x_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

// rule 3: out = keep ? S : Lab2BGR(Lab_o), keep = (protect and M == 0) or (M != 255 and Lab_o == Lab_S on all three bytes). It takes the place of the finish's Lab -> BGR launch
template <int FORM>
__global__ void k_region_compose(const uint8_t* __restrict__ s_bgr, const uint8_t* __restrict__ s_lab, const uint8_t* __restrict__ o_lab, const uint8_t* __restrict__ mask,
                                 size_t n, int protect, const CvtTables* __restrict__ t, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int M = mask[i];
    const int L = o_lab[i * 3], a = o_lab[i * 3 + 1], b = o_lab[i * 3 + 2];
    const bool same = L == s_lab[i * 3] && a == s_lab[i * 3 + 1] && b == s_lab[i * 3 + 2];
    if ((protect && M == 0) || (M != 255 && same)) {
        out[i * 3] = s_bgr[i * 3]; out[i * 3 + 1] = s_bgr[i * 3 + 1]; out[i * 3 + 2] = s_bgr[i * 3 + 2];
        return;
    }
    lab2bgr_px<FORM>(L, a, b, t, out + i * 3);
}

int nctk_region_compose(nct_ctx* ctx, hipStream_t s, const uint8_t* s_bgr, const uint8_t* s_lab, const uint8_t* o_lab, const uint8_t* mask, size_t npix, int protect, int form,
                        uint8_t* out_bgr) {
    const void* tab; NCT_TRY(nctk_cvt_tables(ctx, &tab));
    const CvtTables* t = (const CvtTables*)tab;
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (form == 1) hipLaunchKernelGGL(k_region_compose<1>, grid, dim3(256), 0, s, s_bgr, s_lab, o_lab, mask, npix, protect, t, out_bgr);
    else hipLaunchKernelGGL(k_region_compose<0>, grid, dim3(256), 0, s, s_bgr, s_lab, o_lab, mask, npix, protect, t, out_bgr);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ---- reference region masks (SPEC §6.12): what stands between the pulled masks P_k,l (k_vote.hip: k_pull_vote) and the mix and compose above. Streams, one thread per pixel.
// rules 3 and 4: P_l(p) = P_label(p),l(p) (a reference without a mask counts as 255; label null: reference 0) into p_out, and the level mask M_l = min(P_l, Ms_l)
// into m_out — one launch for both; either output nullable, ms null = 255
struct region_pulled { const uint8_t* p[NCT_MAX_REFS]; };
__global__ void k_region_merge(region_pulled pk, const uint8_t* __restrict__ label, const uint8_t* __restrict__ ms, int n, uint8_t* __restrict__ p_out, uint8_t* __restrict__ m_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = label ? min((int)label[i], NCT_MAX_REFS - 1) : 0;
    const uint8_t* src = pk.p[0];
#pragma unroll
    for (int j = 1; j < NCT_MAX_REFS; ++j) src = j == k ? pk.p[j] : src;
    const int v = src ? src[i] : 255;
    if (p_out) p_out[i] = (uint8_t)v;
    if (m_out) m_out[i] = (uint8_t)min(v, ms ? (int)ms[i] : 255);
}

int nctk_region_merge(nct_ctx* ctx, hipStream_t s, const uint8_t* const* pulled, int K, const uint8_t* label, const uint8_t* ms, int n, uint8_t* p_out, uint8_t* m_out) {
    region_pulled pk{};
    for (int k = 0; k < K; ++k) pk.p[k] = pulled[k];
    hipLaunchKernelGGL(k_region_merge, dim3(cdiv(n, 256)), dim3(256), 0, s, pk, K > 1 ? label : nullptr, ms, n, p_out, m_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

// rule 5: F_l = nct_resize_u8c1(P_l -> dh x dw), then the minimum with the source mask at that size (mn nullable). The target is never smaller than the level
// grid, so the 2x area case of k_resize_u8c1 cannot occur: the fixed-point bilinear chain, or — equal sizes — the byte itself
__global__ void k_region_upsize_min(const uint8_t* __restrict__ src, int sh, int sw, const uint8_t* __restrict__ mn, uint8_t* __restrict__ dst, int dh, int dw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)dh * dw) return;
    int v;
    if (sh == dh && sw == dw) v = src[i];
    else {
        const int dy = (int)(i / dw), dx = (int)(i - (size_t)dy * dw);
        v = resize_u8_px(src, sh, sw, dy, dx, dh, dw);
    }
    dst[i] = (uint8_t)(mn ? min(v, (int)mn[i]) : v);
}

int nctk_region_upsize_min(nct_ctx* ctx, hipStream_t s, const uint8_t* src, int sh, int sw, const uint8_t* mn, uint8_t* dst, int dh, int dw) {
    NCT_REQUIRE(dh >= sh && dw >= sw, "region_upsize_min: the target %dx%d is smaller than the level grid %dx%d", dw, dh, sw, sh);
    hipLaunchKernelGGL(k_region_upsize_min, dim3((unsigned)(((size_t)dh * dw + 255) / 256)), dim3(256), 0, s, src, sh, sw, mn, dst, dh, dw);
    NCT_LAUNCH_CHECK();
    return 0;
}
