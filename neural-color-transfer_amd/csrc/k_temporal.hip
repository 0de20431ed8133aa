// k_temporal.hip — the temporal blend of a frame sequence (SPEC §6.3 rule 3), between S1 and the finish of a level. No counterpart in the reference (it treats
// every pair on its own).
// Per level pixel p: D = the integer sum of squared differences of the two frames' 8-bit Lab level images over the 3 x 3 window (taps outside the grid skipped),
// qbar = (double)D / (double)(3 taps), g = 1 / (1 + qbar / sigma^2), tau_p = tau g, and for the pixel's six coefficients x' = x + tau_p (x_prev - x); a NaN in x_prev
// leaves x. All double operations are IEEE, uncontracted (-ffp-contract=off), in exactly that order: numpy float64 gives the same bits.
// One thread per pixel, one launch per level. The 2 x 9 Lab triples are loaded at clamped addresses before the first add (k_select.hip's pattern: the loads are in
// flight together) and the out-of-grid taps masked out of the sum. The coefficients stay in the colour stage's [2][n][3] layout; a thread reads its own twelve doubles
// before it writes its six, so x_out may be x or x_prev. At 700 x 700 the finest level moves 71 MB (+ 3 MB Lab): stream-bound there, launch-bound on the coarse levels.
//
// Motion compensation (SPEC §6.4). k_seq_motion finds per level pixel the displacement m(p) into the previous frame's level image: a 5 x 5 block match on the three
// Lab bytes around a centre doubled from the coarser level's field, integer arithmetic throughout. Both images are one uint32 per pixel (L | a << 8 | b << 16), so a
// tap's three-channel SAD is one v_sad_u8. A 32 x 8 block stages its tile of the current frame with a halo of 2 in LDS (36 x 12 words) and keeps its 25 taps in
// registers across the candidates; the previous frame's packed map (k_seq_pack, kept in the sequence state) is read through global memory at clamped addresses, the
// out-of-grid taps masked out of cost and count. The candidate loops are uniform over the block (only the centre differs per pixel), the tap loops fully unrolled.
// k_seq_blend<true> then reads L_(t-1) and X'_(t-1) at p + m(p): it gathers from other pixels, so x_out may be x but not x_prev.
//
// Propagated frames (SPEC §6.5). k_seq_warp moves the kept coefficients along a field: x_out(p) = x_prev(p + m(p)), the six 64-bit words of the pixel copied as integers
// (a NaN keeps its payload). One thread per pixel: one short2, six gathered words in flight together, six plain stores; no LDS, no atomics. It gathers, so it runs out of
// place. At 700 x 700 the finest level moves 47 MB + 2 MB of field: stream-bound there, launch-bound on the coarse levels.
//
// The change measure (SPEC §6.7 rule 1). k_seq_change sums, over a level, r(p) = the three-byte SAD of L_t(p) and L_(t-1)(p + m(p)), and counts the pixels with r(p) > T.
// One thread per pixel: the two triples packed into words, one v_sad_u8. A wave's two sums fit one 32-bit word (64 * 765 < 2^16 below, a count <= 64 above), so the wave
// reduces with six lane shifts of one register; the four words of a workgroup meet in LDS, and thread 0 adds the workgroup's sums to the record's two integer fields
// with vector atomics. Integer sums do not depend on the order the workgroups arrive in: the record is exact and the same on every run. No float, no second pass.
#include "nct_internal.h"
#include "nct_device.h"

template <bool MC>
__global__ void __launch_bounds__(256) k_seq_blend(const double* x, const double* x_prev, const uint8_t* __restrict__ lab, const uint8_t* __restrict__ lab_prev, int h, int w,
                                                   double tau, double sigma2, double* x_out, double* __restrict__ tau_map, const short2* __restrict__ field) {
    const int n = h * w;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, px = i - y * w;
    int my = 0, mx = 0;
    if constexpr (MC) {
        // a field of k_seq_motion keeps p + m inside the grid; one from elsewhere is clamped to that, so no address below depends on what the caller passed
        const short2 m = field[i];
        my = clampi(y + m.x, 0, h - 1) - y; mx = clampi(px + m.y, 0, w - 1) - px;
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
    int cur[9][3], old[9][3];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) { cur[t][c] = lab[off[t] + c]; old[t][c] = lab_prev[offp[t] + c]; }
    // the coefficients are independent of the Lab taps: their loads go out before the sum needs anything
    const int ip = MC ? (y + my) * w + px + mx : i;
    double xv[6], pv[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const size_t e = (size_t)(q / 3) * 3 * n + (size_t)3 * i + q % 3;
        const size_t ep = (size_t)(q / 3) * 3 * n + (size_t)3 * ip + q % 3;
        xv[q] = x[e]; pv[q] = x_prev[ep];
    }
    int D = 0, taps = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int d = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int v = cur[t][c] - old[t][c]; d += v * v; }
        if (in[t]) { D += d; taps += 1; }
    }
    const double g = seq_gain(D, taps, sigma2);             // nct_device.h: shared with k_select_hold (SPEC §6.18 rule 3)
    const double tp = tau * g;
    if (tau_map) tau_map[i] = tp;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const size_t e = (size_t)(q / 3) * 3 * n + (size_t)3 * i + q % 3;
        const double b = xv[q] + tp * (pv[q] - xv[q]);
        x_out[e] = (pv[q] != pv[q]) ? xv[q] : b;
    }
}

// [n][3] Lab bytes -> [n] words L | a << 8 | b << 16
__global__ void __launch_bounds__(256) k_seq_pack(const uint8_t* __restrict__ lab, int n, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (uint32_t)lab[3 * i] | ((uint32_t)lab[3 * i + 1] << 8) | ((uint32_t)lab[3 * i + 2] << 16);
}

// SPEC §6.5 rule 3. The words stay in the colour stage's [2][n][3] layout; the vector is clamped component-wise as in k_seq_blend<true>
__global__ void __launch_bounds__(256) k_seq_warp(const unsigned long long* __restrict__ x_prev, int h, int w, const short2* __restrict__ field, unsigned long long* __restrict__ x_out) {
    const int n = h * w;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, px = i - y * w;
    const short2 m = field[i];
    const int ip = clampi(y + m.x, 0, h - 1) * w + clampi(px + m.y, 0, w - 1);
    unsigned long long v[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = x_prev[(size_t)(q / 3) * 3 * n + (size_t)3 * ip + q % 3];
#pragma unroll
    for (int q = 0; q < 6; ++q) x_out[(size_t)(q / 3) * 3 * n + (size_t)3 * i + q % 3] = v[q];
}

// SPEC §6.7 rule 1; the vector is clamped component-wise as in k_seq_warp. rec is zeroed on the stream before the launch. A thread past the grid loads nothing and adds 0
__global__ void __launch_bounds__(256) k_seq_change(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ lab_prev, int h, int w, const short2* __restrict__ field, int T,
                                                    nct_seq_change_rec* __restrict__ rec) {
    __shared__ uint32_t s_wave[4];
    const int n = h * w;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v = 0;                                            // r(p) | (r(p) > T) << 16
    if (i < n) {
        int ip = i;
        if (field) {
            const int y = i / w, px = i - y * w;
            const short2 m = field[i];
            ip = clampi(y + m.x, 0, h - 1) * w + clampi(px + m.y, 0, w - 1);
        }
        const uint32_t a = (uint32_t)lab[3 * i] | ((uint32_t)lab[3 * i + 1] << 8) | ((uint32_t)lab[3 * i + 2] << 16);
        const uint32_t b = (uint32_t)lab_prev[3 * ip] | ((uint32_t)lab_prev[3 * ip + 1] << 8) | ((uint32_t)lab_prev[3 * ip + 2] << 16);
        const uint32_t r = __builtin_amdgcn_sad_u8(a, b, 0u);
        v = r | ((int)r > T ? 1u << 16 : 0u);
    }
    v += __shfl_down(v, 32); v += __shfl_down(v, 16); v += __shfl_down(v, 8);
    v += __shfl_down(v, 4); v += __shfl_down(v, 2); v += __shfl_down(v, 1);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sad = 0; uint32_t changed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { sad += s_wave[k] & 0xffffu; changed += s_wave[k] >> 16; }
        if (sad) atomicAdd((unsigned long long*)&rec->sad, sad);
        if (changed) atomicAdd(&rec->changed, changed);
        if (blockIdx.x == 0) rec->pixels = (uint32_t)n;
    }
}

#define MC_BW 32
#define MC_BH 8
#define MC_P 2                                  // patch half-width: 5 x 5 taps
#define MC_TW (MC_BW + 2 * MC_P)
#define MC_TH (MC_BH + 2 * MC_P)

// cost and tap count of displacement (my, mx) at pixel (y, px): SPEC §6.4 rule 2. cur: the pixel's 25 taps of the current frame, qmask: bit t = tap t is inside the grid.
// The validity of the 25 taps is kept as bits of one register (row bits x column bits), not as 25 lane masks: the count is one popcount, a tap's SAD is multiplied by its bit
__device__ __forceinline__ void mc_cost(const uint32_t (&cur)[25], uint32_t qmask, const uint32_t* __restrict__ prev, int y, int px, int h, int w, int my, int mx, int& cost, int& cnt) {
    int rowoff[5], col[5];
    uint32_t rexp = 0, cb = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const int ry = y + t - MC_P + my, rx = px + t - MC_P + mx;
        rexp |= (uint32_t)ry < (uint32_t)h ? 31u << (5 * t) : 0u;
        cb |= (uint32_t)rx < (uint32_t)w ? 1u << t : 0u;
        rowoff[t] = clampi(ry, 0, h - 1) * w; col[t] = clampi(rx, 0, w - 1);
    }
    const uint32_t valid = qmask & rexp & (cb * 0x108421u);
    uint32_t old[25];
#pragma unroll
    for (int t = 0; t < 25; ++t) old[t] = prev[rowoff[t / 5] + col[t % 5]];
    uint32_t c = 0;
#pragma unroll
    for (int t = 0; t < 25; ++t) c += __builtin_amdgcn_sad_u8(cur[t], old[t], 0u) * ((valid >> t) & 1u);
    cost = (int)c; cnt = __builtin_popcount(valid);
}

__global__ void __launch_bounds__(MC_BW * MC_BH) k_seq_motion(const uint8_t* __restrict__ lab, const uint32_t* __restrict__ prev, int h, int w, const short2* __restrict__ parent,
                                                              int ph, int pw, int R, int penalty, short2* __restrict__ m_out) {
    __shared__ uint32_t tile[MC_TH][MC_TW];
    const int x0 = blockIdx.x * MC_BW, y0 = blockIdx.y * MC_BH;
    const int tid = threadIdx.y * MC_BW + threadIdx.x;
    for (int e = tid; e < MC_TH * MC_TW; e += MC_BW * MC_BH) {
        const int r = e / MC_TW, c = e - r * MC_TW;
        const int o = 3 * (clampi(y0 - MC_P + r, 0, h - 1) * w + clampi(x0 - MC_P + c, 0, w - 1));     // outside the grid: any in-grid word, the tap is masked
        tile[r][c] = (uint32_t)lab[o] | ((uint32_t)lab[o + 1] << 8) | ((uint32_t)lab[o + 2] << 16);
    }
    __syncthreads();
    const int px = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (px >= w || y >= h) return;
    uint32_t cur[25], qmask = 0;
#pragma unroll
    for (int t = 0; t < 25; ++t) {
        const int ty = t / 5, tx = t % 5;
        cur[t] = tile[threadIdx.y + ty][threadIdx.x + tx];
        const int qy = y + ty - MC_P, qx = px + tx - MC_P;
        if (qy >= 0 && qy < h && qx >= 0 && qx < w) qmask |= 1u << t;
    }
    // rule 1: the centre, twice the coarser level's vector, clamped so that p + c is inside
    int cy = 0, cx = 0;
    if (parent) {
        const short2 m = parent[min(y >> 1, ph - 1) * pw + min(px >> 1, pw - 1)];
        cy = clampi(y + 2 * m.x, 0, h - 1) - y; cx = clampi(px + 2 * m.y, 0, w - 1) - px;
    }
    // rule 3: (0, 0) first, then the ring |dy| + |dx| = s for s = 1 .. 2R, each by ascending (dy, dx); the loops are uniform over the block
    int bcost, bn;
    mc_cost(cur, qmask, prev, y, px, h, w, cy, cx, bcost, bn);
    int bK = bcost, by = cy, bx = cx;
    for (int s = 1; s <= 2 * R; ++s) {
        for (int dy = -R; dy <= R; ++dy) {
            const int adx = s - abs(dy);
            if (adx < 0 || adx > R) continue;
            for (int sg = adx ? -1 : 1; sg <= 1; sg += 2) {
                const int my = cy + dy, mx = cx + sg * adx;
                const bool adm = y + my >= 0 && y + my < h && px + mx >= 0 && px + mx < w;
                int cost, cnt;
                mc_cost(cur, qmask, prev, y, px, h, w, my, mx, cost, cnt);
                const int K = cost + penalty * cnt * s;
                if (adm && K * bn < bK * cnt) { bK = K; bn = cnt; by = my; bx = mx; }
            }
        }
    }
    m_out[y * w + px] = make_short2((short)by, (short)bx);
}

int nctk_seq_blend(nct_ctx* ctx, hipStream_t s, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                   double* x_out, double* tau_map, const int16_t* field) {
    NCT_REQUIRE(x && x_prev && lab && lab_prev && x_out, "seq_blend: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_blend: grid %dx%d out of range", w, h);
    NCT_REQUIRE(tau >= 0.0 && tau < 1.0, "seq_blend: tau must be in [0, 1) (got %g)", tau);
    NCT_REQUIRE(sigma > 0.0 && sigma <= 1.7976931348623157e308, "seq_blend: sigma must be finite and positive (got %g)", sigma);
    if (field) {
        // with a field the kernel reads x_prev at other pixels than the one it writes: any overlap of the two maps is refused
        const size_t bytes = sizeof(double) * 6 * (size_t)h * w;
        NCT_REQUIRE((const char*)x_out + bytes <= (const char*)x_prev || (const char*)x_prev + bytes <= (const char*)x_out, "seq_blend: with a motion field x_out must not alias x_prev");
        hipLaunchKernelGGL(k_seq_blend<true>, dim3(cdiv(h * w, 256)), dim3(256), 0, s, x, x_prev, lab, lab_prev, h, w, tau, sigma * sigma, x_out, tau_map, (const short2*)field);
    } else
        hipLaunchKernelGGL(k_seq_blend<false>, dim3(cdiv(h * w, 256)), dim3(256), 0, s, x, x_prev, lab, lab_prev, h, w, tau, sigma * sigma, x_out, tau_map, (const short2*)nullptr);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nctk_seq_pack(nct_ctx* ctx, hipStream_t s, const uint8_t* lab, int n, uint32_t* out) {
    NCT_REQUIRE(lab && out && n >= 1, "seq_pack: bad arguments");
    hipLaunchKernelGGL(k_seq_pack, dim3(cdiv(n, 256)), dim3(256), 0, s, lab, n, out);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nctk_seq_motion(nct_ctx* ctx, hipStream_t s, const uint8_t* lab, const uint32_t* prev_packed, int h, int w, const int16_t* parent, int ph, int pw, int R, int penalty,
                    int16_t* m_out) {
    NCT_REQUIRE(lab && prev_packed && m_out, "seq_motion: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_motion: grid %dx%d out of range", w, h);
    NCT_REQUIRE(!parent || (ph >= 1 && pw >= 1 && ph <= 4096 && pw <= 4096), "seq_motion: parent grid %dx%d out of range", pw, ph);
    NCT_REQUIRE(R >= 0 && R <= 8, "seq_motion: the search radius must be in [0, 8] (got %d)", R);
    NCT_REQUIRE(penalty >= 0 && penalty <= 255, "seq_motion: the penalty must be in [0, 255] (got %d)", penalty);
    hipLaunchKernelGGL(k_seq_motion, dim3(cdiv(w, MC_BW), cdiv(h, MC_BH)), dim3(MC_BW, MC_BH), 0, s, lab, prev_packed, h, w, (const short2*)parent, ph, pw, R, penalty, (short2*)m_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nctk_seq_warp(nct_ctx* ctx, hipStream_t s, const double* x_prev, int h, int w, const int16_t* field, double* x_out) {
    NCT_REQUIRE(x_prev && field && x_out, "seq_warp: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_warp: grid %dx%d out of range", w, h);
    // the kernel reads x_prev at other pixels than the one it writes: any overlap of the two maps is refused
    const size_t bytes = sizeof(double) * 6 * (size_t)h * w;
    NCT_REQUIRE((const char*)x_out + bytes <= (const char*)x_prev || (const char*)x_prev + bytes <= (const char*)x_out, "seq_warp: x_out must not alias x_prev");
    hipLaunchKernelGGL(k_seq_warp, dim3(cdiv(h * w, 256)), dim3(256), 0, s, (const unsigned long long*)x_prev, h, w, (const short2*)field, (unsigned long long*)x_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nctk_seq_change(nct_ctx* ctx, hipStream_t s, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, const int16_t* field, int threshold, nct_seq_change_rec* rec) {
    NCT_REQUIRE(lab && lab_prev, "seq_change: null image");
    NCT_REQUIRE(rec, "seq_change: null out");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_change: grid %dx%d out of range", w, h);
    NCT_REQUIRE(threshold >= 0 && threshold <= 765, "seq_change: the threshold must be in [0, 765] (got %d)", threshold);
    NCT_HIP(hipMemsetAsync(rec, 0, sizeof *rec, s));
    hipLaunchKernelGGL(k_seq_change, dim3(cdiv(h * w, 256)), dim3(256), 0, s, lab, lab_prev, h, w, (const short2*)field, threshold, rec);
    NCT_LAUNCH_CHECK();
    return 0;
}
