// k_colorsolve.hip — local colour transfer on the GPU: T1 local statistics, T2 confidence weights, S1 nonlocal
// least squares (truncated CG), U1 upsample + roughness, S2 edge-aware WLS smoothing (PCG), A1 apply. T1..S1 are nctk_color_nonlocal, U1..A1 "the finish"
// (nctk_color_finish): on the pipeline's levels it targets the working grid, in the full-resolution entry the original source (SPEC §6.1); between the two: nct_seq.cpp.
// Reference: ColorTransfer::transfer_color_downsample ColorTransfer.cpp:1180-1478 and what it calls:
//   stats loop :1194-1265 (+ build_accumTable_downsample :425-455), weights :1302-1357,
//   solve_nonlocal_downsample_gpu_gradient :548-949 -> solve_ls_cg_gpu SparseSolver_GPU.cu:3-198,
//   upsample_color_coefficients_bilinear :457-490, solve_WLS_roughness_cpu :951-1125 -> PARDISO SparseSolver_CPU.cpp:104-286.
//
// MI355X design (the reference assembles CSR on the host, ships it to the GPU three times, forms A^T A with SpGEMM and
// factorises a 490k x 490k matrix with PARDISO on the CPU at every level):
//  * nothing leaves the device. All vectors are fp64, interleaved [pixel][3 Lab channels], a-part then b-part;
//  * S1 is matrix free: A has <= 2 non-zeros per row, so A^T A is (a) a 2x2 data block per pixel and channel,
//    (b) twice the 5-point graph Laplacian with weights g^2 and (c) the kNN graph Laplacian. The out-edges come from the
//    [n][8] kNN table, the in-edges from a radix-sorted reverse adjacency. The three Lab channels run in lock step
//    with their own CG scalars; it is the SAME truncated, un-preconditioned recurrence started from the local-stats
//    guess and stopped by the 50/100 iteration cap — the iterate count is part of the result;
//  * S2: the 5-point SPD system is solved for its 6 right-hand sides in lock step by preconditioned CG
//    (the reference's direct solve is exact, so any converged solver is result-equivalent);
//  * all reductions are two-stage with fixed-shape trees => run-to-run deterministic.
// Roofline: HBM streaming of a handful of fp64 vectors per iteration (latency/launch bound at the coarse levels).
#include "nct_internal.h"
#include "nct_device.h"
#include "nct_detmath.h"
#include "nct_reduce.h"
#include "nct_pixel.h"                               // LAB_D, apply_px
#include <cstring>
#include <cstdio>
#include <rocprim/device/device_radix_sort.hpp>   // rocPRIM directly (no CUB-compatibility layer)


// ================================================================= T1 local statistics
__global__ void k_local_stats(const uint8_t* __restrict__ cnt, const uint8_t* __restrict__ stl, int h, int w, double eps,
                              double* __restrict__ a, double* __restrict__ b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const int sx = max(x - 1, 0), sy = max(y - 1, 0), ex = min(x + 2, w), ey = min(y + 2, h);
    const int cSum = (ex - sx) * (ey - sy);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        long long cs = 0, cs2 = 0, ss = 0, ss2 = 0;
        for (int yy = sy; yy < ey; ++yy)
            for (int xx = sx; xx < ex; ++xx) {
                const int cv = cnt[((size_t)yy * w + xx) * 3 + c], sv = stl[((size_t)yy * w + xx) * 3 + c];
                cs += cv; cs2 += cv * cv; ss += sv; ss2 += sv * sv;
            }
        const double cm = (double)cs / (double)cSum;
        double cvr = (double)cs2 / (double)cSum - cm * cm; cvr = cvr > 0.0 ? cvr : 0.0;
        double csd = sqrt(cvr); csd = csd > 0.0 ? csd : 0.0;
        const double sm = (double)ss / (double)cSum;
        double svr = (double)ss2 / (double)cSum - sm * sm; svr = svr > 0.0 ? svr : 0.0;
        double ssd = sqrt(svr); ssd = ssd > 0.0 ? ssd : 0.0;
        const double av = ssd / (csd + eps);
        a[(size_t)i * 3 + c] = av;
        b[(size_t)i * 3 + c] = (sm - cm * av) * (1.0 / 255.0);
    }
}

// ================================================================= T2 weights
__device__ __forceinline__ unsigned f2ord(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__global__ void k_minmax_f(const float* __restrict__ v, int n, unsigned* __restrict__ mm) {
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    // a NaN (the matching error of a dead feature pixel: `norm` divides by a zero norm, GeneralizedPatchMatch.cu:276-277) takes part in neither extreme, exactly like
    // the reference's `if (err2 < minDist)` / `if (err2 > maxDist)` comparisons (ColorTransfer.cpp:1311-1320); its weight then becomes 1e-6 in k_err_weight, which is what
    // the reference's max() — the Windows macro (stdafx.h includes windows.h): ((a) > (b)) ? (a) : (b) — makes of a NaN
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { const float f = v[i]; if (f == f) { const unsigned o = f2ord(f); lo = min(lo, o); hi = max(hi, o); } }
    for (int off = 32; off >= 1; off >>= 1) { lo = min(lo, (unsigned)__shfl_xor((int)lo, off)); hi = max(hi, (unsigned)__shfl_xor((int)hi, off)); }
    if ((threadIdx.x & 63) == 0) { atomicMin(&mm[0], lo); atomicMax(&mm[1], hi); }
}
__global__ void k_err_weight(const float* __restrict__ err, int n, const unsigned* __restrict__ mm, double* __restrict__ weight) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double mn = (double)ord2f(mm[0]), mx = (double)ord2f(mm[1]);
    const double e = ((double)err[i] - mn) / (mx - mn);
    const double wv = 1.0 - e;
    weight[i] = wv > 1e-6 ? wv : 1e-6;
}

// gradient weights g = sqrt(lamda / (|dL|^alpha + 1e-4)) of the L channel of an 8-bit Lab image (compute_gradientMat)
__global__ void k_gradient_weights(const uint8_t* __restrict__ lab, int h, int w, double lamda, double alpha, double* __restrict__ gx, double* __restrict__ gy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const double val = LAB_D(lab[(size_t)i * 3]);
    double vx = 0.0, vy = 0.0;
    if (x + 1 < w) { const double g = LAB_D(lab[(size_t)(i + 1) * 3]) - val; vx = sqrt(lamda / (nct_pow(fabs(g), alpha) + 0.0001)); }
    if (y + 1 < h) { const double g = LAB_D(lab[(size_t)(i + w) * 3]) - val; vy = sqrt(lamda / (nct_pow(fabs(g), alpha) + 0.0001)); }
    gx[i] = vx; gy[i] = vy;
}

// ================================================================= U1 roughness / A1 apply
__global__ void k_roughness(const double* __restrict__ a, const double* __restrict__ b, const uint8_t* __restrict__ lab, int n, double* __restrict__ rough) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double nc = LAB_D(lab[(size_t)i * 3 + 2]) * a[(size_t)i * 3 + 2] + b[(size_t)i * 3 + 2];     // only channel 2 survives (quirk 5)
    rough[i] = (nc < 0 || nc > 1) ? 1e-6 : 1.0;
}
__global__ void k_apply(const double* __restrict__ a, const double* __restrict__ b, const uint8_t* __restrict__ lab, int n, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 3) return;
    out[i] = apply_px(a[i], b[i], lab[i]);
}

// ================================================================= S2 WLS: (diag(r) + L) x = r x0, 6 right-hand sides

__global__ void k_wls_system(const double* __restrict__ gx, const double* __restrict__ gy, const double* __restrict__ rough, int H, int W,
                             double* __restrict__ diag, double* __restrict__ wx, double* __restrict__ wy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    double a00 = 0.0, ex = 0.0, ey = 0.0;
    a00 += rough[i];
    if (x + 1 < W) { const double g = gx[i] * gx[i]; a00 += g; ex = g; }
    if (x > 0) { const double g = gx[i - 1] * gx[i - 1]; a00 += g; }
    if (y + 1 < H) { const double g = gy[i] * gy[i]; a00 += g; ey = g; }
    if (y > 0) { const double g = gy[i - W] * gy[i - W]; a00 += g; }
    diag[i] = a00; wx[i] = ex; wy[i] = ey;
}
// ================================================================= orchestration
#define LCHK() NCT_LAUNCH_CHECK()

// ================================================================= the finish: U1, roughness, S2, A1 on a target grid H x W >= h x w
// x: [2][h*w][3] coefficients after S1 on the level grid; Hw x Ww: the working size the pyramid runs at (the pipeline's "full" grid of every
// level). The pipeline's own levels pass H x W = Hw x Ww; the full-resolution entry passes the original source (SPEC §6.1). Index arithmetic is
// int for pixels (N <= 2^26) and size_t for every element offset past 3 N.
int nctk_color_finish(nct_ctx* ctx, hipStream_t s, const double* x, int h, int w, int Hw, int Ww, const uint8_t* s_lab_full, int H, int W,
                      const nct_color_params& prm, uint8_t* out_lab_full, const nct_color_debug* dbg, const nct_finish_up* up) {
    NCT_REQUIRE(h > 0 && w > 0 && H >= h && W >= w && H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS,
                "color finish: target %dx%d outside [%dx%d, %d per side, %lld px]", W, H, w, h, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    // ---------------- U1: bilinear upsample to full resolution + roughness
    const int n = h * w, N = H * W, nbL = cdiv(N, 256);
    const double* xa = x; const double* xb = x + (size_t)3 * n;
    DevBuf<double> X(ctx, (size_t)6 * N), rough(ctx, N);
    if (!X.ok() || !rough.ok()) return NCT_ERR_HIP;
    double* Xa = X; double* Xb = (double*)X + (size_t)3 * N;
    if (W > w || H > h) {
        NCT_TRY(nctk_resize_f64c3(ctx, s, xa, h, w, Xa, H, W));
        NCT_TRY(nctk_resize_f64c3(ctx, s, xb, h, w, Xb, H, W));
    } else {
        NCT_HIP(hipMemcpyAsync(X, x, sizeof(double) * (size_t)6 * N, hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_roughness, dim3(nbL), dim3(256), 0, s, (const double*)Xa, (const double*)Xb, s_lab_full, N, (double*)rough); LCHK();
    if (dbg) { NCT_TRY(dbg_copy(ctx, s, dbg->ab_up, X, (size_t)6 * N)); NCT_TRY(dbg_copy(ctx, s, dbg->rough, rough, N)); }
    // ---------------- S2: WLS (k_wls_mg.hip)
    {
        // ColorTransfer.cpp:1418-1424 with the target's own ratio; the x4 of a level that already has the working size stays tied to the working size (SPEC §6.1)
        const double r = (double)((long long)H * W) / (double)((long long)h * w);
        double lamda = prm.wls_lambda_init * r;
        if (h == Hw && w == Ww) lamda *= 4;
        DevBuf<double> gx(ctx, N), gy(ctx, N), diag(ctx, N), wx(ctx, N), wy(ctx, N);
        if (!gx.ok() || !gy.ok() || !diag.ok() || !wx.ok() || !wy.ok()) return NCT_ERR_HIP;
        hipLaunchKernelGGL(k_gradient_weights, dim3(nbL), dim3(256), 0, s, s_lab_full, H, W, lamda, prm.wls_alpha, (double*)gx, (double*)gy); LCHK();
        hipLaunchKernelGGL(k_wls_system, dim3(nbL), dim3(256), 0, s, (const double*)gx, (const double*)gy, (const double*)rough, H, W, (double*)diag, (double*)wx, (double*)wy); LCHK();
        int wit[6] = {0, 0, 0, 0, 0, 0};
        NCT_TRY(ctx->mark(s, nct_stage_tag(NCT_ST_COLOR, ctx->tm_level)));
        NCT_TRY(nctk_wls_solve_mg(ctx, s, X, rough, wx, wy, H, W, ctx->wls_rtol, wit));
        NCT_TRY(ctx->mark(s, nct_stage_tag(NCT_ST_WLS, ctx->tm_level)));
        if (dbg && dbg->wls_iters) for (int q = 0; q < 6; ++q) dbg->wls_iters[q] = wit[q];
    }
    if (dbg) NCT_TRY(dbg_copy(ctx, s, dbg->ab_wls, X, (size_t)6 * N));
    // ---------------- A1
    hipLaunchKernelGGL(k_apply, dim3(cdiv(3 * N, 256)), dim3(256), 0, s, (const double*)Xa, (const double*)Xb, s_lab_full, N, out_lab_full); LCHK();
    // ---------------- SPEC §6.8: the same smoothed maps onto the original source
    // with a mask (SPEC §6.13 rule 4) the compose with the original source rides in the same pass; guided (SPEC §6.10), s_lab_full is the guide
    if (up) NCT_TRY(nctk_finish_up(ctx, s, X, s_lab_full, H, W, *up));
    return 0;
}

// ================================================================= T1, T2, S1 on the level grid h x w: the level's coefficients into b.x
// H x W: the working size (S1's dWeight). b stays the caller's until the finish that reads b.x has been enqueued
int nctk_color_nonlocal(nct_ctx* ctx, hipStream_t s, const float* err, const uint8_t* s_lab_level, const uint8_t* g_lab_level, const int* knn_id, const double* knn_w,
                        int layer, int h, int w, int H, int W, const nct_color_params& prm, nct_color_bufs& b, const nct_color_debug* dbg, const nct_s1_graph* graph) {
    const int n = h * w;
    const int nbl = cdiv(n, 256);
    // ---------------- T1 + T2
    if (!b.x.alloc(ctx, (size_t)6 * n) || !b.weight.alloc(ctx, n) || !b.mm.alloc(ctx, 2)) return NCT_ERR_HIP;
    double* const x = b.x; double* const weight = b.weight; unsigned* const mm = b.mm;
    double* xa = x; double* xb = x + (size_t)3 * n;
    hipLaunchKernelGGL(k_local_stats, dim3(nbl), dim3(256), 0, s, s_lab_level, g_lab_level, h, w, prm.eps, xa, xb); LCHK();
    if (dbg) NCT_TRY(dbg_copy(ctx, s, dbg->ab_local, x, (size_t)6 * n));
    NCT_HIP(hipMemsetD32Async((hipDeviceptr_t)mm, (int)0xFFFFFFFFu, 1, s));
    NCT_HIP(hipMemsetD32Async((hipDeviceptr_t)(mm + 1), 0, 1, s));
    hipLaunchKernelGGL(k_minmax_f, dim3(128), dim3(256), 0, s, err, n, mm); LCHK();
    hipLaunchKernelGGL(k_err_weight, dim3(nbl), dim3(256), 0, s, err, n, (const unsigned*)mm, weight); LCHK();
    NCT_TRY(ctx->mark(s, nct_stage_tag(NCT_ST_COLOR, ctx->tm_level)));
    // ---------------- S1 (k_s1.hip)
    const double normFactor = (double)(W * H) / (double)(w * h);
    {
        DevBuf<double> gx(ctx, n), gy(ctx, n);
        if (!gx.ok() || !gy.ok()) return NCT_ERR_HIP;
        // lambda / alpha / dWeight arrive as float in the reference signature (ColorTransfer.cpp:548-550)
        const float lambda_f = (float)prm.local_weight, alpha_f = (float)prm.wls_alpha, dWeight_f = (float)normFactor;
        hipLaunchKernelGGL(k_gradient_weights, dim3(nbl), dim3(256), 0, s, s_lab_level, h, w, (double)lambda_f, (double)alpha_f, (double*)gx, (double*)gy); LCHK();
        nct_s1_graph_bufs gb;
        if (!graph) {
            // no prebuilt graph part (the host entry point nct_local_color_transfer): build it here, on this stream; the host does not know the hub block count
            if (!gb.alloc(ctx, n)) return NCT_ERR_HIP;
            NCT_TRY(nctk_s1_graph_build(ctx, s, knn_id, knn_w, sqrt(prm.nonlocal_weight / prm.k_num), gb.view(-1, -1), nullptr));
        }
        NCT_TRY(nctk_s1_solve(ctx, s, graph ? *graph : gb.view(-1, -1), knn_id, weight, dWeight_f, s_lab_level, g_lab_level, gx, gy, layer, h, w, x, dbg ? dbg->cg_iters : nullptr));
    }
    NCT_TRY(ctx->mark(s, nct_stage_tag(NCT_ST_NONLOCAL, ctx->tm_level)));
    return dbg ? dbg_copy(ctx, s, dbg->ab_nonlocal, x, (size_t)6 * n) : 0;
}
