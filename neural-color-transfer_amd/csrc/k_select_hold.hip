// k_select_hold.hip — the held reference selection of a frame sequence over several references (SPEC §6.18 rules 1-6) and the label carry of a propagated frame.
// No counterpart in the reference (it ships neither several references nor sequences).
// Per level pixel p: score_k = k_select.hip's 3 x 3 sum of E_k in double, n = the window taps inside the grid, f = the lowest k of the smallest score;
// j = the label the previous frame kept at p + m(p) (m: the level's field of SPEC §6.4, clamped component-wise; none: 0); g = k_seq_blend's gain on (L_t, L_(t-1)) through
// the same m, by the one device function both kernels call (nct_device.h: seq_gain); margin = (hold g) (double)n; the label is f where j >= K or
// score_f < score_j - margin, else j. The label, G_label's three bytes and E_label's fp32 word go out, f and the margin where they are asked for. All double operations
// are IEEE, uncontracted (-ffp-contract=off), in exactly that order: numpy float64 gives the same bits.
// One thread per pixel, one launch per level, no LDS, no atomics. It follows k_select_reference and k_seq_blend: every address is clamped into its map, the taps outside
// the grid are masked out of the sums afterwards, and all K x 9 error words, the 2 x 9 Lab triples, the field vector and the kept label are loaded before the first add,
// so the loads are in flight together. The K map pointers travel by value in the argument block. The kept label is read at another pixel than the one written: the
// launcher refuses a label map that overlaps the kept one.
// Per level pixel it reads 4 K B of error words (each word nine times, from cache), 6 B of Lab, 4 B of field, 1 B of label and 3 B of the selected guidance image,
// and writes 1 + 3 + 4 B (+ 1 + 8 B when the report is asked for): at 700 x 700, K = 2: 14.7 MB, K = 4: 18.6 MB on the finest level. Launch-bound on the coarse levels, stream-bound at the finest.
// k_label_carry: label_out(p) = label_prev(p + m(p)), the vector clamped as in k_seq_warp; one byte per thread.
#include "nct_internal.h"
#include "nct_device.h"
#include <cmath>

struct hold_maps { const uint32_t* err[NCT_MAX_REFS]; const uint8_t* guide[NCT_MAX_REFS]; };

template <int K, bool MC>
__global__ void __launch_bounds__(256) k_select_hold(hold_maps m, int h, int w, const uint8_t* __restrict__ prev_label, const uint8_t* __restrict__ lab,
                                                     const uint8_t* __restrict__ lab_prev, const short2* __restrict__ field, double hold, double sigma2,
                                                     uint8_t* __restrict__ label, uint8_t* __restrict__ guide_out, uint32_t* __restrict__ err_out,
                                                     uint8_t* __restrict__ free_label, double* __restrict__ margin_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, px = i - y * w;
    int my = 0, mx = 0;
    if constexpr (MC) {
        // a field of k_seq_motion keeps p + m inside the grid; one from elsewhere is clamped to that, so no address below depends on what the caller passed
        const short2 v = field[i];
        my = clampi(y + v.x, 0, h - 1) - y; mx = clampi(px + v.y, 0, w - 1) - px;
    }
    int off[9], offp[9]; bool in[9], inp[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int qy = y + t / 3 - 1, qx = px + t % 3 - 1;
        in[t] = qy >= 0 && qy < h && qx >= 0 && qx < w;
        off[t] = clampi(qy, 0, h - 1) * w + clampi(qx, 0, w - 1);
        inp[t] = in[t]; offp[t] = off[t];
        if constexpr (MC) {
            const int ry = qy + my, rx = qx + mx;
            inp[t] = in[t] && ry >= 0 && ry < h && rx >= 0 && rx < w;
            offp[t] = clampi(ry, 0, h - 1) * w + clampi(rx, 0, w - 1);
        }
    }
    uint32_t e[K][9];                       // fp32 words: the selected one is copied out as it came in
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int t = 0; t < 9; ++t) e[k][t] = m.err[k][off[t]];
    int cur[9][3], old[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) { cur[t][c] = lab[3 * off[t] + c]; old[t][c] = lab_prev[3 * offp[t] + c]; }
    const int j = prev_label[(y + my) * w + px + mx];
    // rule 1: the scores, the free label and the taps inside the grid
    double score[K];
    int f = 0, n = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) n += in[t] ? 1 : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double sc = 0.0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float v = __uint_as_float(e[k][t]);
            if (in[t]) sc += (v != v) ? 0.0 : (double)v;
        }
        score[k] = sc;
    }
    double score_f = score[0];
#pragma unroll
    for (int k = 1; k < K; ++k) if (score[k] < score_f) { f = k; score_f = score[k]; }
    // rule 3: the gain, k_seq_blend's sums
    int D = 0, taps = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int d = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int v = cur[t][c] - old[t][c]; d += v * v; }
        if (inp[t]) { D += d; taps += 1; }
    }
    const double g = seq_gain(D, taps, sigma2);
    const double margin = (hold * g) * (double)n;
    // rule 5: the kept label stays unless the free one is better by more than the margin
    double score_j = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) if (k == j) score_j = score[k];
    const int lbl = (j >= K || score_f < score_j - margin) ? f : j;
    uint32_t word = e[0][4];
    const uint8_t* gsel = m.guide[0];
#pragma unroll
    for (int k = 1; k < K; ++k) if (k == lbl) { word = e[k][4]; gsel = m.guide[k]; }
    if (label) label[i] = (uint8_t)lbl;
    if (free_label) free_label[i] = (uint8_t)f;
    if (margin_out) margin_out[i] = margin;
    if (err_out) err_out[i] = word;
    if (guide_out && gsel) {
        const uint8_t b0 = gsel[3 * (size_t)i], b1 = gsel[3 * (size_t)i + 1], b2 = gsel[3 * (size_t)i + 2];
        guide_out[3 * (size_t)i] = b0; guide_out[3 * (size_t)i + 1] = b1; guide_out[3 * (size_t)i + 2] = b2;
    }
}

// SPEC §6.18 rule 7; the vector is clamped component-wise as in k_seq_warp
__global__ void __launch_bounds__(256) k_label_carry(const uint8_t* __restrict__ label_prev, int h, int w, const short2* __restrict__ field, uint8_t* __restrict__ label_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, px = i - y * w;
    const short2 v = field[i];
    label_out[i] = label_prev[clampi(y + v.x, 0, h - 1) * w + clampi(px + v.y, 0, w - 1)];
}

struct hold_args { int h, w; const uint8_t *prev_label, *lab, *lab_prev; const short2* field; double hold, sigma2; uint8_t *label, *guide_out; uint32_t* err_out; uint8_t* free_label; double* margin; };

template <int K>
static void launch_hold(hipStream_t s, const hold_maps& m, const hold_args& a) {
    const dim3 grid(cdiv(a.h * a.w, 256)), block(256);
    if (a.field)
        hipLaunchKernelGGL((k_select_hold<K, true>), grid, block, 0, s, m, a.h, a.w, a.prev_label, a.lab, a.lab_prev, a.field, a.hold, a.sigma2, a.label, a.guide_out, a.err_out, a.free_label, a.margin);
    else
        hipLaunchKernelGGL((k_select_hold<K, false>), grid, block, 0, s, m, a.h, a.w, a.prev_label, a.lab, a.lab_prev, a.field, a.hold, a.sigma2, a.label, a.guide_out, a.err_out, a.free_label, a.margin);
}

bool nct_seq_hold_ok(double hold) { return std::isfinite(hold) && hold >= 0.0 && hold <= 2.0; }

int nct_select_hold_check(nct_ctx* ctx, const char* who, const void* const* err, const void* const* guide, int K, int h, int w, const void* prev_label, const void* lab,
                          const void* lab_prev, double hold, double sigma, const void* guide_out) {
    NCT_REQUIRE(K >= 1 && K <= NCT_MAX_REFS, "%s: K must be in [1, %d] (got %d)", who, NCT_MAX_REFS, K);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "%s: grid %dx%d out of range", who, w, h);
    NCT_REQUIRE(err && (guide || !guide_out), "%s: null map list", who);
    for (int k = 0; k < K; ++k) NCT_REQUIRE(err[k] && (!guide_out || guide[k]), "%s: null map of reference %d", who, k);
    NCT_REQUIRE(prev_label, "%s: null prev_label", who);
    NCT_REQUIRE(lab && lab_prev, "%s: null Lab image", who);
    NCT_REQUIRE(nct_seq_hold_ok(hold), "%s: hold must be finite and in [0, 2] (got %g)", who, hold);
    NCT_REQUIRE(nct_guided_sigma_ok(sigma), "%s: sigma must be finite and positive (got %g)", who, sigma);
    return NCT_OK;
}

int nctk_select_hold(nct_ctx* ctx, hipStream_t s, const float* const* err, const uint8_t* const* guide, int K, int h, int w, const uint8_t* prev_label, const uint8_t* lab,
                     const uint8_t* lab_prev, const int16_t* field, double hold, double sigma, uint8_t* label, uint8_t* guide_out, float* err_out, uint8_t* free_label,
                     double* margin) {
    NCT_TRY(nct_select_hold_check(ctx, "select_reference_hold", (const void* const*)err, (const void* const*)guide, K, h, w, prev_label, lab, lab_prev, hold, sigma, guide_out));
    // the rule gathers the kept label from other pixels than the one it writes: any overlap of the two label maps is refused
    const size_t bytes = (size_t)h * w;
    NCT_REQUIRE(!label || (const char*)label + bytes <= (const char*)prev_label || (const char*)prev_label + bytes <= (const char*)label, "select_reference_hold: label must not alias prev_label");
    hold_maps m{};
    for (int k = 0; k < K; ++k) { m.err[k] = (const uint32_t*)err[k]; m.guide[k] = guide_out ? guide[k] : nullptr; }
    const hold_args a{h, w, prev_label, lab, lab_prev, (const short2*)field, hold, sigma * sigma, label, guide_out, (uint32_t*)err_out, free_label, margin};
    switch (K) {
        case 1: launch_hold<1>(s, m, a); break;
        case 2: launch_hold<2>(s, m, a); break;
        case 3: launch_hold<3>(s, m, a); break;
        case 4: launch_hold<4>(s, m, a); break;
        case 5: launch_hold<5>(s, m, a); break;
        case 6: launch_hold<6>(s, m, a); break;
        case 7: launch_hold<7>(s, m, a); break;
        default: launch_hold<8>(s, m, a); break;
    }
    NCT_LAUNCH_CHECK();
    return 0;
}

int nctk_label_carry(nct_ctx* ctx, hipStream_t s, const uint8_t* label_prev, int h, int w, const int16_t* field, uint8_t* label_out) {
    NCT_REQUIRE(label_prev && field && label_out, "label_carry: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "label_carry: grid %dx%d out of range", w, h);
    const size_t bytes = (size_t)h * w;
    NCT_REQUIRE((const char*)label_out + bytes <= (const char*)label_prev || (const char*)label_prev + bytes <= (const char*)label_out, "label_carry: label_out must not alias label_prev");
    hipLaunchKernelGGL(k_label_carry, dim3(cdiv(h * w, 256)), dim3(256), 0, s, label_prev, h, w, (const short2*)field, label_out);
    NCT_LAUNCH_CHECK();
    return 0;
}
