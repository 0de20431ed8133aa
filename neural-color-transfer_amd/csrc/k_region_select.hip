// k_region_select.hip — region selection from strokes (SPEC §6.16): the kernels that turn one VGG19 tap of the source and a stroke map into a matte on the tap grid.
//   k_feat_quantize   rule 2: N1 of the raw HWC tap (k_normalize's summation, bit for bit) and q = rint(u * 32767) as int16, [cells][C]
//   k_sel_flags       rule 3: per source pixel one atomicOr on its cell's word (bit 0: an IN pixel, bit 1: an OUT pixel); most pixels are unmarked and issue nothing
//   k_sel_words       the scan's input: one 64-bit word per cell, low half 1 for an inside seed cell, high half 1 for an outside one; one rocPRIM exclusive scan of
//                     cells + 1 words then holds both raster ranks per cell and, in its last word, both totals
//   k_sel_assign      the subsample rule, the cell codes of nct_region_select_stages.cell and the kept seeds' cell indices (inside first, then outside)
//   k_sel_rows        the kept seeds' rows gathered into one contiguous [n_in + n_out][C] int16 array
//   k_region_score    rule 4, the hot path: an integer "GEMM with a max epilogue"
//   k_sel_stamp       rule 6: IN pixels 255, OUT pixels 0
//
// k_region_score on the MI355X. cells x (n_in + n_out) x C multiply-adds, every operand an int16, every sum an exact int32 (SPEC §6.16 rule 2). One workgroup of 256
// threads owns a tile of SC_TQ = 128 query cells and walks ALL seeds in chunks of SC_TS = 64, so that the maxima never leave the workgroup: no cross-workgroup reduction,
// no atomic. The two classes are one list (inside first): a chunk may straddle the class border, the epilogue sorts each seed column by its index, and only the last chunk
// of the list is padded — 64 + 64 seeds cost two chunks, not four. Channels are staged through LDS SC_KC = 64 at a time: 128 + 64 rows of 128 B. The threads form a
// 16 x 16 grid, thread (tq, ts) holds an 8 x 4 block of int32 accumulators for the queries tq + 16 i and the seeds ts + 16 j. Per 16 bytes of channels it issues
// 8 + 4 ds_read_b128 and 8 * 4 * 4 = 128 v_dot2c_i32_i16 (__builtin_amdgcn_sdot2): 10.7 dot instructions per LDS read, where a 4 x 4 block would have 8.
// LDS layout: a row stride of 144 B (128 + one 16-B slot of padding). ds_read_b128 is served in groups of 16 lanes and banks (address / 4) mod 64: a group holds all 16 values
// of tq (lanes with the same tq read the same address: a broadcast), the rows tq + 16 i start 36 tq dwords apart, and 36 tq mod 64 runs over the 16 multiples of 4, so the
// 16 four-bank slots are distinct; the seed rows of a group are at most two, 36 dwords apart. Staging is register-prefetched: the 8-byte global loads of stage t + 1 are
// issued in front of the dot products of stage t (8-byte units, so that C need only be a multiple of 4; they come from L2: the seed list is at most 8 MB and every
// workgroup reads all of it). A K tail (C % 64) and rows past the ends are staged as zeros and add nothing.
// The epilogue: per thread the running maxima of its 8 queries per class, then one pass through LDS (row stride 17 words) in which thread t < 128 reduces query t over the 16
// seed columns and applies rule 4 in 64 bits: d = s_in - s_out, m = clamp(128 + ((d * sharpness + 2^29) >> 30), 0, 255), an arithmetic shift being floor division.
// Arithmetic count and what was measured: DESIGN.md §3.21.
#include "nct_internal.h"
#include "nct_device.h"
#include <rocprim/device/device_scan.hpp>   // rocPRIM directly (no CUB-compatibility layer)

// ---------------------------------------------------------------- rule 2: quantise
__device__ __forceinline__ short quant16(float u) {
    const float t = u * 32767.0f;
    return __builtin_isfinite(u) ? (short)(int)rintf(t) : (short)0;
}

// k_normalize's frame (k_feat.hip): one 16-lane DPP row per pixel, lane v owns the float4 chunks v, v + 16, …, one fmaf chain per lane, the 16-lane rotate-and-add
__global__ __launch_bounds__(256) void k_feat_quantize(const float* __restrict__ src, short* __restrict__ dst, int C, int HW) {
    int pix = blockIdx.x * 16 + (threadIdx.x >> 4);
    int v = threadIdx.x & 15;
    bool live = pix < HW;
    int p = live ? pix : HW - 1;
    const float4* s4 = reinterpret_cast<const float4*>(src + (size_t)p * C);
    int nchunk = C >> 2;
    float acc = 0.f;
    for (int j = v; j < nchunk; j += 16) { float4 x = s4[j]; acc = dot4_acc(x, x, acc); }
    float d = sqrtf(row16_sum(acc));
    if (!live) return;
    short4* d4 = reinterpret_cast<short4*>(dst + (size_t)p * C);
    for (int j = v; j < nchunk; j += 16) {
        float4 x = s4[j];
        d4[j] = make_short4(quant16(x.x / d), quant16(x.y / d), quant16(x.z / d), quant16(x.w / d));
    }
}

int nctk_feat_quantize(nct_ctx* ctx, hipStream_t s, const float* src_hwc, int16_t* dst, int C, int HW) {
    NCT_REQUIRE(C > 0 && (C & 3) == 0, "feat_quantize: C=%d must be a positive multiple of 4", C);
    hipLaunchKernelGGL(k_feat_quantize, dim3(cdiv(HW, 16)), dim3(256), 0, s, src_hwc, (short*)dst, C, HW);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- rule 3: seed cells
__global__ void k_sel_flags(const uint8_t* __restrict__ strokes, int h, int w, int shift, int wt, unsigned* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const uint8_t t = strokes[i];
    if (t != NCT_STROKE_IN && t != NCT_STROKE_OUT) return;
    const int y = i / w, x = i - y * w;
    atomicOr(&flags[(y >> shift) * wt + (x >> shift)], t == NCT_STROKE_IN ? 1u : 2u);
}

__global__ void k_sel_words(const unsigned* __restrict__ flags, int cells, unsigned long long* __restrict__ words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > cells) return;
    const unsigned f = i < cells ? flags[i] : 0u;
    words[i] = f == 1u ? 1ull : (f == 2u ? 1ull << 32 : 0ull);
}

// The seed of raster rank i among the n of its class is kept iff floor((i + 1) k / n) > floor(i k / n), k = min(n, max_seeds); floor(i k / n) counts the kept seeds in
// front of it and so is its slot. n <= max_seeds: k = n, every seed is kept in its rank's slot
__global__ void k_sel_assign(const unsigned* __restrict__ flags, const unsigned long long* __restrict__ pre, int cells, unsigned n_in, unsigned n_out, unsigned k_in,
                             unsigned k_out, uint8_t* __restrict__ code, int* __restrict__ idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const unsigned f = flags[i];
    uint8_t c = 0;
    if (f == 3u) c = 5;
    else if (f != 0u) {
        const bool in = f == 1u;
        const unsigned long long rank = in ? (pre[i] & 0xffffffffull) : (pre[i] >> 32);
        const unsigned long long n = in ? n_in : n_out, k = in ? k_in : k_out;
        const unsigned long long lo = rank * k / n, hi = (rank + 1) * k / n;
        const bool kept = hi > lo;
        c = in ? (kept ? 1 : 3) : (kept ? 2 : 4);
        if (kept) idx[(in ? 0u : k_in) + (unsigned)lo] = i;
    }
    code[i] = c;
}

// one 16-lane row per kept seed, 8-byte units
__global__ __launch_bounds__(256) void k_sel_rows(const short* __restrict__ q, const int* __restrict__ idx, int n, int C, short* __restrict__ seeds) {
    const int sd = blockIdx.x * 16 + (threadIdx.x >> 4), v = threadIdx.x & 15;
    if (sd >= n) return;
    const uint2* src = reinterpret_cast<const uint2*>(q + (size_t)idx[sd] * C);
    uint2* dst = reinterpret_cast<uint2*>(seeds + (size_t)sd * C);
    for (int j = v; j < (C >> 2); j += 16) dst[j] = src[j];
}

int nctk_sel_cells(nct_ctx* ctx, hipStream_t s, const uint8_t* strokes, int h, int w, int tap, unsigned* flags, unsigned long long* pre /* [cells + 1] */) {
    const int shift = tap - 1, ht = ((h - 1) >> shift) + 1, wt = ((w - 1) >> shift) + 1, cells = ht * wt;
    DevBuf<unsigned long long> words(ctx, (size_t)cells + 1);
    if (!words.ok()) return NCT_ERR_HIP;
    NCT_HIP(hipMemsetAsync(flags, 0, sizeof(unsigned) * cells, s));
    hipLaunchKernelGGL(k_sel_flags, dim3(cdiv(h * w, 256)), dim3(256), 0, s, strokes, h, w, shift, wt, flags);
    NCT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sel_words, dim3(cdiv(cells + 1, 256)), dim3(256), 0, s, (const unsigned*)flags, cells, (unsigned long long*)words);
    NCT_LAUNCH_CHECK();
    size_t scan_bytes = 0;
    NCT_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (const unsigned long long*)words, pre, 0ull, (size_t)cells + 1, rocprim::plus<unsigned long long>(), s));
    DevBuf<char> tmp(ctx, scan_bytes);
    if (!tmp.ok()) return NCT_ERR_HIP;
    NCT_HIP(rocprim::exclusive_scan((void*)(char*)tmp, scan_bytes, (const unsigned long long*)words, pre, 0ull, (size_t)cells + 1, rocprim::plus<unsigned long long>(), s));
    return 0;
}

int nctk_sel_seeds(nct_ctx* ctx, hipStream_t s, const int16_t* q, const unsigned* flags, const unsigned long long* pre, int cells, int C, unsigned n_in, unsigned n_out,
                   unsigned k_in, unsigned k_out, uint8_t* code, int* idx /* [k_in + k_out] */, int16_t* seeds /* [k_in + k_out][C] */) {
    hipLaunchKernelGGL(k_sel_assign, dim3(cdiv(cells, 256)), dim3(256), 0, s, flags, pre, cells, n_in, n_out, k_in, k_out, code, idx);
    NCT_LAUNCH_CHECK();
    const int n = (int)(k_in + k_out);
    hipLaunchKernelGGL(k_sel_rows, dim3(cdiv(n, 16)), dim3(256), 0, s, (const short*)q, (const int*)idx, n, C, (short*)seeds);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- rule 4: score
#define SC_NJ 4                                 // seed columns per thread (8 query rows)
#define SC_KC 64                                // int16 channels per stage
#define SC_TQ 128
#define SC_TS (16 * SC_NJ)
#define SC_ROW (SC_KC * 2 + 16)                 // bytes between staged rows
#define SC_UPR (SC_KC / 4)                      // 8-byte units per staged row
#define SC_QU (SC_TQ * SC_UPR / 256)            // 8-byte units a thread stages per stage: queries 8, seeds 4
#define SC_SU (SC_TS * SC_UPR / 256)
#define SC_RED 17                               // words between the reduction's rows

typedef short sc_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int sc_dot2(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(sc_short2, a), __builtin_bit_cast(sc_short2, b), c, false);
}

__global__ __launch_bounds__(256) void k_region_score(const short* __restrict__ q, int cells, int C, const short* __restrict__ seeds_in, int n_in,
                                                      const short* __restrict__ seeds_out, int n_out, long long sharpness, long long floor_score,
                                                      const uint8_t* __restrict__ code /* nullable */, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[(SC_TQ + SC_TS) * SC_ROW];
    unsigned char* const lq = lds;
    unsigned char* const ls = lds + SC_TQ * SC_ROW;
    const int tid = threadIdx.x, tq = tid & 15, ts = tid >> 4;
    const int q0 = blockIdx.x * SC_TQ;
    const int n_tot = n_in + n_out;
    const int nk = (C + SC_KC - 1) / SC_KC, nchunk = (n_tot + SC_TS - 1) / SC_TS, nstage = nk * nchunk;

    uint2 rq[SC_QU], rs[SC_SU];
    // the loads of stage t: unit u = tid + 256 i is row u / SC_UPR, channels 4 (u % SC_UPR) … + 3 of the stage's SC_KC
    auto load = [&](int t) {
        const int chunk = t / nk, k0 = (t - chunk * nk) * SC_KC, s0 = chunk * SC_TS;
#pragma unroll
        for (int i = 0; i < SC_QU; ++i) {
            const int u = tid + 256 * i, row = u / SC_UPR, k = k0 + ((u % SC_UPR) << 2);
            rq[i] = make_uint2(0u, 0u);
            if (q0 + row < cells && k < C) rq[i] = *reinterpret_cast<const uint2*>(q + (size_t)(q0 + row) * C + k);
        }
#pragma unroll
        for (int i = 0; i < SC_SU; ++i) {
            const int u = tid + 256 * i, g = s0 + (u / SC_UPR), k = k0 + ((u % SC_UPR) << 2);
            rs[i] = make_uint2(0u, 0u);
            if (g < n_tot && k < C) rs[i] = *reinterpret_cast<const uint2*>(g < n_in ? seeds_in + (size_t)g * C + k : seeds_out + (size_t)(g - n_in) * C + k);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < SC_QU; ++i) { const int u = tid + 256 * i; *reinterpret_cast<uint2*>(lq + (u / SC_UPR) * SC_ROW + ((u % SC_UPR) << 3)) = rq[i]; }
#pragma unroll
        for (int i = 0; i < SC_SU; ++i) { const int u = tid + 256 * i; *reinterpret_cast<uint2*>(ls + (u / SC_UPR) * SC_ROW + ((u % SC_UPR) << 3)) = rs[i]; }
    };

    int mi[8], mo[8], acc[8][SC_NJ];
#pragma unroll
    for (int i = 0; i < 8; ++i) { mi[i] = INT_MIN; mo[i] = INT_MIN; }
    load(0);
    for (int t = 0; t < nstage; ++t) {
        const int chunk = t / nk, ks = t - chunk * nk;
        __syncthreads();                                   // the previous stage's reads are done
        store();
        __syncthreads();
        if (t + 1 < nstage) load(t + 1);
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < SC_NJ; ++j) acc[i][j] = 0;
        }
#pragma unroll 1
        for (int kk = 0; kk < SC_KC * 2; kk += 16) {
            uint4 a[8], b[SC_NJ];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = *reinterpret_cast<const uint4*>(lq + (tq + 16 * i) * SC_ROW + kk);
#pragma unroll
            for (int j = 0; j < SC_NJ; ++j) b[j] = *reinterpret_cast<const uint4*>(ls + (ts + 16 * j) * SC_ROW + kk);
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < SC_NJ; ++j) {
                    int c = acc[i][j];
                    c = sc_dot2(a[i].x, b[j].x, c); c = sc_dot2(a[i].y, b[j].y, c); c = sc_dot2(a[i].z, b[j].z, c); c = sc_dot2(a[i].w, b[j].w, c);
                    acc[i][j] = c;
                }
        }
        if (ks == nk - 1) {
            // the max epilogue of this chunk: seed column j of this thread is seed g of the list, inside below n_in, padding from n_tot on
#pragma unroll
            for (int j = 0; j < SC_NJ; ++j) {
                const int g = chunk * SC_TS + ts + 16 * j;
                if (g < n_in) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) mi[i] = max(mi[i], acc[i][j]);
                } else if (g < n_tot) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) mo[i] = max(mo[i], acc[i][j]);
                }
            }
        }
    }
    __syncthreads();
    int* const red_in = reinterpret_cast<int*>(lds);
    int* const red_out = red_in + SC_TQ * SC_RED;          // 2 * 128 * 17 words = 17408 B of the 27648
#pragma unroll
    for (int i = 0; i < 8; ++i) { red_in[(tq + 16 * i) * SC_RED + ts] = mi[i]; red_out[(tq + 16 * i) * SC_RED + ts] = mo[i]; }
    __syncthreads();
    if (tid >= SC_TQ || q0 + tid >= cells) return;
    int s_in = INT_MIN, s_out = INT_MIN;
#pragma unroll
    for (int j = 0; j < 16; ++j) { s_in = max(s_in, red_in[tid * SC_RED + j]); s_out = max(s_out, red_out[tid * SC_RED + j]); }
    const long long d = (long long)s_in - (n_out > 0 ? (long long)s_out : floor_score);
    long long m = 128 + ((d * sharpness + (1LL << 29)) >> 30);
    m = m < 0 ? 0 : (m > 255 ? 255 : m);
    if (code) {
        const uint8_t c = code[q0 + tid];
        if (c == 1 || c == 3) m = 255; else if (c == 2 || c == 4) m = 0;
    }
    out[q0 + tid] = (uint8_t)m;
}

int nct_region_score_check(nct_ctx* ctx, const char* who, const void* q, int cells, int C, const void* seeds_in, int n_in, const void* seeds_out, int n_out, int sharpness,
                           int floor_permille, const void* score_out) {
    NCT_REQUIRE(q, "%s: null q", who);
    NCT_REQUIRE(seeds_in, "%s: null seeds_in", who);
    NCT_REQUIRE(score_out, "%s: null score_out", who);
    NCT_REQUIRE(cells >= 1 && cells <= (1 << 24), "%s: cells must be in [1, 2^24] (got %d)", who, cells);
    NCT_REQUIRE(C >= 4 && C <= 4096 && (C & 3) == 0, "%s: C must be a multiple of 4 in [4, 4096] (got %d)", who, C);
    NCT_REQUIRE(n_in >= 1 && n_in <= 65536, "%s: n_in must be in [1, 65536] (got %d)", who, n_in);
    NCT_REQUIRE(n_out >= 0 && n_out <= 65536, "%s: n_out must be in [0, 65536] (got %d)", who, n_out);
    NCT_REQUIRE(n_out == 0 || seeds_out, "%s: null seeds_out with n_out = %d", who, n_out);
    NCT_REQUIRE(sharpness >= 1 && sharpness <= 65536, "%s: sharpness must be in [1, 65536] (got %d)", who, sharpness);
    NCT_REQUIRE(floor_permille >= 0 && floor_permille <= 1000, "%s: floor_permille must be in [0, 1000] (got %d)", who, floor_permille);
    return 0;
}

int nctk_region_score(nct_ctx* ctx, hipStream_t s, const int16_t* q, int cells, int C, const int16_t* seeds_in, int n_in, const int16_t* seeds_out, int n_out, int sharpness,
                      int floor_permille, const uint8_t* code, uint8_t* score_out) {
    NCT_TRY(nct_region_score_check(ctx, "region_score", q, cells, C, seeds_in, n_in, seeds_out, n_out, sharpness, floor_permille, score_out));
    // the kernel reads the rows in 8-byte units
    NCT_REQUIRE(((uintptr_t)q & 7) == 0, "region_score: q must be 8-byte aligned");
    NCT_REQUIRE(((uintptr_t)seeds_in & 7) == 0, "region_score: seeds_in must be 8-byte aligned");
    NCT_REQUIRE(n_out == 0 || ((uintptr_t)seeds_out & 7) == 0, "region_score: seeds_out must be 8-byte aligned");
    const long long floor_score = (long long)floor_permille * (1LL << 30) / 1000;
    hipLaunchKernelGGL(k_region_score, dim3(cdiv(cells, SC_TQ)), dim3(256), 0, s, (const short*)q, cells, C, (const short*)seeds_in, n_in, (const short*)seeds_out, n_out,
                       (long long)sharpness, floor_score, code, score_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- rule 6: stamp
__global__ void k_sel_stamp(const uint8_t* __restrict__ strokes, size_t n, uint8_t* __restrict__ m) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t t = strokes[i];
    if (t == NCT_STROKE_IN) m[i] = 255; else if (t == NCT_STROKE_OUT) m[i] = 0;
}

int nctk_sel_stamp(nct_ctx* ctx, hipStream_t s, const uint8_t* strokes, size_t n, uint8_t* m) {
    hipLaunchKernelGGL(k_sel_stamp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, strokes, n, m);
    NCT_LAUNCH_CHECK();
    return 0;
}
