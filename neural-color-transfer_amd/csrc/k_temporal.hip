// k_temporal.hip — the temporal blend of a frame sequence (SPEC §6.3 rule 3), between S1 and the finish of a level. No counterpart in the reference (it treats
// every pair on its own).
// Per level pixel p: D = the integer sum of squared differences of the two frames' 8-bit Lab level images over the 3 x 3 window (taps outside the grid skipped),
// qbar = (double)D / (double)(3 taps), g = 1 / (1 + qbar / sigma^2), tau_p = tau g, and for the pixel's six coefficients x' = x + tau_p (x_prev - x); a NaN in x_prev
// leaves x. All double operations are IEEE, uncontracted (-ffp-contract=off), in exactly that order: numpy float64 gives the same bits.
// One thread per pixel, one launch per level. The 2 x 9 Lab triples are loaded at clamped addresses before the first add (k_select.hip's pattern: the loads are in
// flight together) and the out-of-grid taps masked out of the sum. The coefficients stay in the colour stage's [2][n][3] layout; a thread reads its own twelve doubles
// before it writes its six, so x_out may be x or x_prev. At 700 x 700 the finest level moves 71 MB (+ 3 MB Lab): stream-bound there, launch-bound on the coarse levels.
#include "nct_internal.h"
#include "nct_device.h"

__global__ void __launch_bounds__(256) k_seq_blend(const double* x, const double* x_prev, const uint8_t* __restrict__ lab, const uint8_t* __restrict__ lab_prev, int h, int w,
                                                   double tau, double sigma2, double* x_out, double* __restrict__ tau_map) {
    const int n = h * w;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, px = i - y * w;
    int off[9]; bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int qy = y + t / 3 - 1, qx = px + t % 3 - 1;
        in[t] = qy >= 0 && qy < h && qx >= 0 && qx < w;
        off[t] = 3 * (clampi(qy, 0, h - 1) * w + clampi(qx, 0, w - 1));
    }
    int cur[9][3], old[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) { cur[t][c] = lab[off[t] + c]; old[t][c] = lab_prev[off[t] + c]; }
    // the coefficients are independent of the Lab taps: their loads go out before the sum needs anything
    double xv[6], pv[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const size_t e = (size_t)(q / 3) * 3 * n + (size_t)3 * i + q % 3;
        xv[q] = x[e]; pv[q] = x_prev[e];
    }
    int D = 0, taps = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int d = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int v = cur[t][c] - old[t][c]; d += v * v; }
        if (in[t]) { D += d; taps += 1; }
    }
    const double qbar = (double)D / (double)(3 * taps);
    const double g = 1.0 / (1.0 + qbar / sigma2);
    const double tp = tau * g;
    if (tau_map) tau_map[i] = tp;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const size_t e = (size_t)(q / 3) * 3 * n + (size_t)3 * i + q % 3;
        const double b = xv[q] + tp * (pv[q] - xv[q]);
        x_out[e] = (pv[q] != pv[q]) ? xv[q] : b;
    }
}

int nctk_seq_blend(nct_ctx* ctx, hipStream_t s, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                   double* x_out, double* tau_map) {
    NCT_REQUIRE(x && x_prev && lab && lab_prev && x_out, "seq_blend: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_blend: grid %dx%d out of range", w, h);
    NCT_REQUIRE(tau >= 0.0 && tau < 1.0, "seq_blend: tau must be in [0, 1) (got %g)", tau);
    NCT_REQUIRE(sigma > 0.0 && sigma <= 1.7976931348623157e308, "seq_blend: sigma must be finite and positive (got %g)", sigma);
    hipLaunchKernelGGL(k_seq_blend, dim3(cdiv(h * w, 256)), dim3(256), 0, s, x, x_prev, lab, lab_prev, h, w, tau, sigma * sigma, x_out, tau_map);
    NCT_LAUNCH_CHECK();
    return 0;
}
