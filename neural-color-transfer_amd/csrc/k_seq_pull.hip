// k_seq_pull.hip — the held pull of a frame sequence with a reference region mask (SPEC §6.19 rules 2-4). No counterpart in the reference (it ships neither masks
// nor sequences).
// Per level pixel p: P = the pulled byte of the pixel's label (k_region_merge's rule: a reference without a mask counts as 255, a label past the list is clamped);
// j = the byte the previous frame kept at p + m(p) (m: the level's field of SPEC §6.4, clamped component-wise; none: 0); tau_p = tau g, g = k_seq_blend's gain on
// (L_t, L_(t-1)) through the same m, by the one device function the three kernels call (nct_device.h: seq_gain); P' = (uint8) rint((double)P + tau_p ((double)j - (double)P));
// M = min(P', the source level mask or 255). All double operations are IEEE, uncontracted (-ffp-contract=off), in exactly that order: numpy float64 gives the same bits.
// tau_p is in [0, 1), so P' lies between P and j and the conversion cannot leave the byte.
// One thread per pixel, 256 per workgroup, one launch per level, no LDS, no atomics. It follows k_select_hold: every address is clamped into its map, the taps outside
// the grid are masked out of the sums afterwards, and the label, the K pulled bytes, the 2 x 9 Lab triples, the field vector, the kept byte and the source mask byte are
// loaded before the first add. The K map pointers travel by value in the argument block. Neighbouring threads read and write neighbouring bytes of a row. The kept map
// is read at another pixel than the one written: the launcher refuses a p_out that overlaps it.
// Per level pixel it reads 1 B of label, up to K B of pulled masks, 6 B of Lab (each byte nine times, from cache), 4 B of field, 1 B of kept mask and 1 B of source
// mask, and writes 1 + 1 (+ 1) B: at 700 x 700, K = 2: 7.4 MB on the finest level. Launch-bound on every level but the finest.
#include "nct_internal.h"
#include "nct_device.h"
#include <cmath>

struct pull_maps { const uint8_t* p[NCT_MAX_REFS]; };

template <bool MC>
__global__ void __launch_bounds__(256) k_seq_pull_hold(pull_maps pk, const uint8_t* __restrict__ label, const uint8_t* __restrict__ prev, const uint8_t* __restrict__ lab,
                                                       const uint8_t* __restrict__ lab_prev, const short2* __restrict__ field, const uint8_t* __restrict__ ms, int h, int w,
                                                       double tau, double sigma2, uint8_t* __restrict__ p_out, uint8_t* __restrict__ m_out, uint8_t* __restrict__ p_free) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, px = i - y * w;
    int my = 0, mx = 0;
    if constexpr (MC) {
        // a field of k_seq_motion keeps p + m inside the grid; one from elsewhere is clamped to that, so no address below depends on what the caller passed
        const short2 v = field[i];
        my = clampi(y + v.x, 0, h - 1) - y; mx = clampi(px + v.y, 0, w - 1) - px;
    }
    int off[9], offp[9]; bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int qy = y + t / 3 - 1, qx = px + t % 3 - 1;
        in[t] = qy >= 0 && qy < h && qx >= 0 && qx < w;
        off[t] = 3 * (clampi(qy, 0, h - 1) * w + clampi(qx, 0, w - 1));
        offp[t] = off[t];
        if constexpr (MC) {
            const int ry = qy + my, rx = qx + mx;
            in[t] = in[t] && ry >= 0 && ry < h && rx >= 0 && rx < w;
            offp[t] = 3 * (clampi(ry, 0, h - 1) * w + clampi(rx, 0, w - 1));
        }
    }
    // rule 2: the pulled byte of the pixel's label, as k_region_merge reads it
    const int k = label ? min((int)label[i], NCT_MAX_REFS - 1) : 0;
    const uint8_t* src = pk.p[0];
#pragma unroll
    for (int q = 1; q < NCT_MAX_REFS; ++q) src = q == k ? pk.p[q] : src;
    const int P = src ? (int)src[i] : 255;
    const int j = prev[(y + my) * w + px + mx];
    const int s_mask = ms ? (int)ms[i] : 255;
    int cur[9][3], old[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) { cur[t][c] = lab[off[t] + c]; old[t][c] = lab_prev[offp[t] + c]; }
    // rule 3: the blend's weight, k_seq_blend's sums
    int D = 0, taps = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int d = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int v = cur[t][c] - old[t][c]; d += v * v; }
        if (in[t]) { D += d; taps += 1; }
    }
    const double g = seq_gain(D, taps, sigma2);
    const double tp = tau * g;
    const double held = (double)P + tp * ((double)j - (double)P);
    const int Ph = (int)(uint8_t)rint(held);
    p_out[i] = (uint8_t)Ph;
    if (m_out) m_out[i] = (uint8_t)min(Ph, s_mask);
    if (p_free) p_free[i] = (uint8_t)P;
}

int nct_seq_pull_hold_check(nct_ctx* ctx, const char* who, const void* const* pulled, int K, const void* label, const void* prev, const void* lab, const void* lab_prev, int h, int w,
                            double tau, double sigma, const void* p_out) {
    NCT_REQUIRE(K >= 1 && K <= NCT_MAX_REFS, "%s: K must be in [1, %d] (got %d)", who, NCT_MAX_REFS, K);
    NCT_REQUIRE(h >= 1 && h <= 4096, "%s: h = %d is not in [1, 4096]", who, h);
    NCT_REQUIRE(w >= 1 && w <= 4096, "%s: w = %d is not in [1, 4096]", who, w);
    NCT_REQUIRE(pulled, "%s: pulled is null", who);
    NCT_REQUIRE(label || K == 1, "%s: label is null (K = %d references)", who, K);
    NCT_REQUIRE(prev, "%s: prev is null", who);
    NCT_REQUIRE(lab, "%s: lab is null", who);
    NCT_REQUIRE(lab_prev, "%s: lab_prev is null", who);
    NCT_REQUIRE(p_out, "%s: p_out is null", who);
    NCT_REQUIRE(tau >= 0.0 && tau < 1.0, "%s: tau must be in [0, 1) (got %g)", who, tau);
    NCT_REQUIRE(nct_guided_sigma_ok(sigma), "%s: sigma must be finite and positive (got %g)", who, sigma);
    return NCT_OK;
}

int nctk_seq_pull_hold(nct_ctx* ctx, hipStream_t s, const uint8_t* const* pulled, int K, const uint8_t* label, const uint8_t* prev, const uint8_t* lab, const uint8_t* lab_prev,
                       const int16_t* field, const uint8_t* src_mask, int h, int w, double tau, double sigma, uint8_t* p_out, uint8_t* m_out, uint8_t* p_free) {
    NCT_TRY(nct_seq_pull_hold_check(ctx, "seq_pull_hold", (const void* const*)pulled, K, label, prev, lab, lab_prev, h, w, tau, sigma, p_out));
    // the rule gathers the kept byte from other pixels than the one it writes: any overlap of the two maps is refused
    const size_t bytes = (size_t)h * w;
    NCT_REQUIRE((const char*)p_out + bytes <= (const char*)prev || (const char*)prev + bytes <= (const char*)p_out, "seq_pull_hold: p_out must not alias prev");
    pull_maps pk{};
    for (int k = 0; k < K; ++k) pk.p[k] = pulled[k];
    const dim3 grid(cdiv(h * w, 256)), block(256);
    const uint8_t* lbl = K > 1 ? label : nullptr;
    if (field)
        hipLaunchKernelGGL(k_seq_pull_hold<true>, grid, block, 0, s, pk, lbl, prev, lab, lab_prev, (const short2*)field, src_mask, h, w, tau, sigma * sigma, p_out, m_out, p_free);
    else
        hipLaunchKernelGGL(k_seq_pull_hold<false>, grid, block, 0, s, pk, lbl, prev, lab, lab_prev, (const short2*)nullptr, src_mask, h, w, tau, sigma * sigma, p_out, m_out, p_free);
    NCT_LAUNCH_CHECK();
    return 0;
}
