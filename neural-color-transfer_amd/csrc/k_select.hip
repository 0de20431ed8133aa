// k_select.hip — reference selection of a level with several references (SPEC §6.2 rules 2 and 3).
// Per pixel: score_k = sum of E_k over the 3 x 3 window, in double, dy outer / dx inner, NaN = 0.0, taps outside the grid skipped; label = the lowest k of the
// smallest score; the label, G_label's three bytes and E_label's fp32 word go out. No counterpart in the reference (it ships the single-reference form only).
// One thread per pixel, one launch per level. The K map pointers travel by value in the argument block; all K x 9 taps (clamped addresses, the out-of-grid
// ones masked out of the sum afterwards) are loaded before the first add, so the loads are in flight together. At 700 x 700 and K = 4 the kernel moves
// about 14 MB: it is bound by its launch, nothing cleverer is worth having.
#include "nct_internal.h"
#include "nct_device.h"

struct select_maps { const uint32_t* err[NCT_MAX_REFS]; const uint8_t* guide[NCT_MAX_REFS]; };

template <int K>
__global__ void __launch_bounds__(256) k_select_reference(select_maps m, int h, int w, uint8_t* __restrict__ label, uint8_t* __restrict__ guide_out,
                                                          uint32_t* __restrict__ err_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    int off[9]; bool in[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int qy = y + t / 3 - 1, qx = x + t % 3 - 1;
        in[t] = qy >= 0 && qy < h && qx >= 0 && qx < w;
        off[t] = clampi(qy, 0, h - 1) * w + clampi(qx, 0, w - 1);
    }
    uint32_t e[K][9];                       // fp32 words: the selected one is copied out as it came in
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) e[k][t] = m.err[k][off[t]];
    int best = 0; double best_score = 0.0; uint32_t best_word = e[0][4];
    const uint8_t* g = m.guide[0];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double score = 0.0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = __uint_as_float(e[k][t]);
            if (in[t]) score += (v != v) ? 0.0 : (double)v;
        }
        if (k == 0 || score < best_score) { best = k; best_score = score; best_word = e[k][4]; g = m.guide[k]; }
    }
    if (label) label[i] = (uint8_t)best;
    if (err_out) err_out[i] = best_word;
    if (guide_out && g) {
        const uint8_t b0 = g[3 * (size_t)i], b1 = g[3 * (size_t)i + 1], b2 = g[3 * (size_t)i + 2];
        guide_out[3 * (size_t)i] = b0; guide_out[3 * (size_t)i + 1] = b1; guide_out[3 * (size_t)i + 2] = b2;
    }
}

template <int K>
static void launch_select(hipStream_t s, const select_maps& m, int h, int w, uint8_t* label, uint8_t* guide_out, float* err_out) {
    hipLaunchKernelGGL(k_select_reference<K>, dim3(cdiv(h * w, 256)), dim3(256), 0, s, m, h, w, label, guide_out, (uint32_t*)err_out);
}

int nctk_select_reference(nct_ctx* ctx, hipStream_t s, const float* const* err, const uint8_t* const* guide /*nullable, like guide_out*/, int K, int h, int w,
                          uint8_t* label, uint8_t* guide_out, float* err_out) {
    NCT_REQUIRE(K >= 1 && K <= NCT_MAX_REFS, "select_reference: K must be in [1, %d] (got %d)", NCT_MAX_REFS, K);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "select_reference: grid %dx%d out of range", w, h);
    NCT_REQUIRE(err && (guide || !guide_out), "select_reference: null map list");
    select_maps m{};
    for (int k = 0; k < K; ++k) {
        NCT_REQUIRE(err[k] && (!guide_out || guide[k]), "select_reference: null map of reference %d", k);
        m.err[k] = (const uint32_t*)err[k]; m.guide[k] = guide_out ? guide[k] : nullptr;
    }
    switch (K) {
        case 1: launch_select<1>(s, m, h, w, label, guide_out, err_out); break;
        case 2: launch_select<2>(s, m, h, w, label, guide_out, err_out); break;
        case 3: launch_select<3>(s, m, h, w, label, guide_out, err_out); break;
        case 4: launch_select<4>(s, m, h, w, label, guide_out, err_out); break;
        case 5: launch_select<5>(s, m, h, w, label, guide_out, err_out); break;
        case 6: launch_select<6>(s, m, h, w, label, guide_out, err_out); break;
        case 7: launch_select<7>(s, m, h, w, label, guide_out, err_out); break;
        default: launch_select<8>(s, m, h, w, label, guide_out, err_out); break;
    }
    NCT_LAUNCH_CHECK();
    return 0;
}
