// k_reflib.hip — reference libraries (SPEC §6.21): the kernels that rank a library's entries against one source by how well their VGG19 tap descriptors match.
//   k_feat_quantize8  rule D2: g = F - mu (fp32, mu nullable), N1 of g (k_normalize's summation, bit for bit) and d = rint(u * 127) as int8, [cells][C]
//   k_desc_match      rule D3, the hot path: P = A B^T in int32 on the matrix cores, its row maxima summed per source tile, its column maxima by atomicMax
//   k_desc_sums       rule D3's two sums per entry in int64: the source tiles' forward partials, the entry's column maxima
//
// k_desc_match on the MI355X. Grid (source tiles, entries). One workgroup of 256 threads owns DM_TM = 128 source rows and walks all rows of ONE entry in chunks of DM_TN =
// 128; the channels of both are staged through LDS DM_KC = 128 bytes at a time in 16-byte units (register-prefetched: the global loads of stage t + 1 are issued in front of
// the MFMAs of stage t), a row stride of 144 B: the 16 lanes a ds_read_b128 is served in read rows r … r + 15 at 36 r dwords, and 36 r mod 64 runs over the 16 multiples
// of 4. The four waves form a 2 x 2 grid: wave (wr, wc) owns source rows 64 wr … + 63 and entry rows 64 wc … + 63 of the chunk as 2 x 2 accumulator tiles of
// v_mfma_i32_32x32x32_i8 (__builtin_amdgcn_mfma_i32_32x32x32_i8), so that per 32 channels it issues 2 + 2 ds_read_b128 and 4 MFMAs.
// THE i8 LANE MAP (established with exact integer data: tests/test_gpu_reflib.py G2, an identity block against an asymmetric matrix, both ways round):
//   A operand, 4 VGPRs = 16 int8: lane l (r = l & 31, h = l >> 5) holds A[row r][k = 16 h + j] in byte j = 0 … 15
//   B operand, 4 VGPRs = 16 int8: lane l holds B[k = 16 h + j][col r] in byte j — here B = (entry rows)^T, so the lane reads 16 bytes of ENTRY ROW r at channel 16 h
//   C/D, 16 int32: register i of lane l is row (i & 3) + 8 (i >> 2) + 4 h, col r — the map of every 32 x 32 MFMA on gfx950
// Both operands read the same 16-byte unit of their own row, so only rows-on-lanes and the C/D map can go wrong, and G2 fails for either.
// Forward maxima: acc is masked per lane (an entry row past nb: INT32_MIN) and folded element-wise into 2 x 16 running maxima per lane — register i of a row block keeps
// the maximum over every entry row the lane has seen in its column position; the 32 lanes of a half are reduced ONCE, after the last chunk. Backward maxima: per chunk
// the accumulators are masked per register (a source row past na: INT32_MIN), reduced over the 2 x 16 registers, the two lane halves and, through 1 KB of LDS, the two
// wave rows, then threads 0 … 127 issue one atomicMax each on colmax[entry row]: integer max is exact in any order. Padding (rows past na / nb, channels past C) is staged as
// zeros and never takes part in a maximum: with a centre P can be negative everywhere, a padded zero must not win.
// |d| <= 128 and C <= 4096: every product sum is below 2^26 in magnitude, int32 throughout (SPEC §6.21 D2). Registers, LDS, occupancy and what was measured: DESIGN.md §3.26.
#include "nct_internal.h"
#include "nct_device.h"
#include <climits>

// ---------------------------------------------------------------- rule D2: quantise to int8
__device__ __forceinline__ signed char quant8(float u) {
    const float t = u * 127.0f;
    return __builtin_isfinite(u) ? (signed char)(int)rintf(t) : (signed char)0;
}

// k_feat_quantize's frame (k_region_select.hip): one 16-lane DPP row per cell, lane v owns the float4 chunks v, v + 16, …, one fmaf chain per lane
__global__ __launch_bounds__(256) void k_feat_quantize8(const float* __restrict__ src, const float* __restrict__ center, signed char* __restrict__ dst, int C, int HW) {
    int pix = blockIdx.x * 16 + (threadIdx.x >> 4);
    int v = threadIdx.x & 15;
    bool live = pix < HW;
    int p = live ? pix : HW - 1;
    const float4* s4 = reinterpret_cast<const float4*>(src + (size_t)p * C);
    const float4* c4 = reinterpret_cast<const float4*>(center);
    int nchunk = C >> 2;
    float acc = 0.f;
    for (int j = v; j < nchunk; j += 16) {
        float4 x = s4[j];
        if (center) { float4 m = c4[j]; x = make_float4(x.x - m.x, x.y - m.y, x.z - m.z, x.w - m.w); }
        acc = dot4_acc(x, x, acc);
    }
    float d = sqrtf(row16_sum(acc));
    if (!live) return;
    char4* d4 = reinterpret_cast<char4*>(dst + (size_t)p * C);
    for (int j = v; j < nchunk; j += 16) {
        float4 x = s4[j];
        if (center) { float4 m = c4[j]; x = make_float4(x.x - m.x, x.y - m.y, x.z - m.z, x.w - m.w); }
        d4[j] = make_char4(quant8(x.x / d), quant8(x.y / d), quant8(x.z / d), quant8(x.w / d));
    }
}

int nctk_feat_quantize8(nct_ctx* ctx, hipStream_t s, const float* src_hwc, const float* center, int8_t* dst, int C, int HW) {
    NCT_REQUIRE(C >= 16 && C <= 4096 && (C & 15) == 0, "feat_quantize8: C must be a multiple of 16 in [16, 4096] (got %d)", C);
    hipLaunchKernelGGL(k_feat_quantize8, dim3(cdiv(HW, 16)), dim3(256), 0, s, src_hwc, center, (signed char*)dst, C, HW);
    NCT_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- rule D3: match
#define DM_TM 128                               // source rows per workgroup
#define DM_TN 128                               // entry rows per chunk
#define DM_KC 128                               // int8 channels per stage
#define DM_ROW (DM_KC + 16)                     // bytes between staged rows
#define DM_UPR (DM_KC / 16)                     // 16-byte units per staged row
#define DM_AU (DM_TM * DM_UPR / 256)            // units a thread stages per stage: 4 of the source, 4 of the entry
#define DM_BU (DM_TN * DM_UPR / 256)

typedef int dm_i32x4 __attribute__((ext_vector_type(4)));
typedef int dm_i32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void k_desc_match(const signed char* __restrict__ a, int na, int C, const signed char* __restrict__ rows, const int* __restrict__ offsets,
                                                    long long* __restrict__ fpart /* [entries][tiles] */, int* __restrict__ colmax /* [total rows], INT32_MIN */) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[(DM_TM + DM_TN) * DM_ROW];
    __shared__ int red[2][DM_TN];               // backward: per wave row the chunk's column maxima; forward, at the end: per wave column the tile's row maxima
    unsigned char* const la = lds;
    unsigned char* const lb = lds + DM_TM * DM_ROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x, ntiles = gridDim.x, entry = blockIdx.y;
    const int a0 = tile * DM_TM;
    const int off = offsets[entry], nb = offsets[entry + 1] - off;
    const signed char* const b = rows + (size_t)off * C;
    const int nk = (C + DM_KC - 1) / DM_KC, nchunk = (nb + DM_TN - 1) / DM_TN, nstage = nk * nchunk;

    uint4 ra[DM_AU], rb[DM_BU];
    // the loads of stage t: unit u = tid + 256 i is row u / DM_UPR, channels 16 (u % DM_UPR) … + 15 of the stage's DM_KC
    auto load = [&](int t) {
        const int chunk = t / nk, k0 = (t - chunk * nk) * DM_KC, c0 = chunk * DM_TN;
#pragma unroll
        for (int i = 0; i < DM_AU; ++i) {
            const int u = tid + 256 * i, row = u / DM_UPR, k = k0 + ((u % DM_UPR) << 4);
            ra[i] = make_uint4(0u, 0u, 0u, 0u);
            if (a0 + row < na && k < C) ra[i] = *reinterpret_cast<const uint4*>(a + (size_t)(a0 + row) * C + k);
        }
#pragma unroll
        for (int i = 0; i < DM_BU; ++i) {
            const int u = tid + 256 * i, row = u / DM_UPR, k = k0 + ((u % DM_UPR) << 4);
            rb[i] = make_uint4(0u, 0u, 0u, 0u);
            if (c0 + row < nb && k < C) rb[i] = *reinterpret_cast<const uint4*>(b + (size_t)(c0 + row) * C + k);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < DM_AU; ++i) { const int u = tid + 256 * i; *reinterpret_cast<uint4*>(la + (u / DM_UPR) * DM_ROW + ((u % DM_UPR) << 4)) = ra[i]; }
#pragma unroll
        for (int i = 0; i < DM_BU; ++i) { const int u = tid + 256 * i; *reinterpret_cast<uint4*>(lb + (u / DM_UPR) * DM_ROW + ((u % DM_UPR) << 4)) = rb[i]; }
    };

    dm_i32x16 acc[2][2];                        // [source row block][entry row block]
    int fmax[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 16; ++g) fmax[i][g] = INT_MIN;
    load(0);
    for (int t = 0; t < nstage; ++t) {
        const int chunk = t / nk, ks = t - chunk * nk;
        __syncthreads();                                   // the previous stage's reads are done
        store();
        __syncthreads();
        if (t + 1 < nstage) load(t + 1);
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int g = 0; g < 16; ++g) acc[i][j][g] = 0;
        }
        const int kleft = C - ks * DM_KC, steps = kleft >= DM_KC ? DM_KC / 32 : (kleft + 31) / 32;      // a K tail's all-zero steps are skipped
        for (int kk = 0; kk < steps; ++kk) {
            const int kb = kk * 32 + 16 * h;
            dm_i32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const dm_i32x4*>(la + (64 * wr + 32 * i + r) * DM_ROW + kb);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const dm_i32x4*>(lb + (64 * wc + 32 * j + r) * DM_ROW + kb);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (ks == nk - 1) {
            const int c0 = chunk * DM_TN;
            // forward: this lane's entry rows are c0 + 64 wc + 32 j + r
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bool colv = c0 + 64 * wc + 32 * j + r < nb;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g = 0; g < 16; ++g) fmax[i][g] = max(fmax[i][g], colv ? acc[i][j][g] : INT_MIN);
            }
            // backward: register g of row block i is source row a0 + 64 wr + 32 i + (g & 3) + 8 (g >> 2) + 4 h
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int m = INT_MIN;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        const bool rowv = a0 + 64 * wr + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * h < na;
                        m = max(m, rowv ? acc[i][j][g] : INT_MIN);
                    }
                m = max(m, __shfl_xor(m, 32));
                if (h == 0) red[wr][64 * wc + 32 * j + r] = m;
            }
            __syncthreads();
            if (tid < DM_TN && c0 + tid < nb) {
                const int m = max(red[0][tid], red[1][tid]);
                if (m != INT_MIN) atomicMax(&colmax[off + c0 + tid], m);     // INT32_MIN: no source row of this tile is live — cannot happen, the grid holds live tiles only
            }
        }
    }
    // forward: the 32 lanes of a half hold one source row's maxima over their column positions
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            int m = fmax[i][g];
            m = max(m, __shfl_xor(m, 1)); m = max(m, __shfl_xor(m, 2)); m = max(m, __shfl_xor(m, 4)); m = max(m, __shfl_xor(m, 8)); m = max(m, __shfl_xor(m, 16));
            fmax[i][g] = m;
        }
    __syncthreads();                                       // the last chunk's reads of red are done
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) red[wc][64 * wr + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * h] = fmax[i][g];
    }
    __syncthreads();
    if (tid < 64) {
        long long s = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = tid + 64 * i;
            if (a0 + row < na) s += (long long)max(red[0][row], red[1][row]);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
        if (tid == 0) fpart[(size_t)entry * ntiles + tile] = s;
    }
}

// one workgroup per entry: fwd[k] = the sum of its tiles' partials, bwd[k] = the sum of its rows' column maxima, both int64
__global__ __launch_bounds__(256) void k_desc_sums(const long long* __restrict__ fpart, int ntiles, const int* __restrict__ colmax, const int* __restrict__ offsets,
                                                   long long* __restrict__ fwd, long long* __restrict__ bwd) {
    __shared__ long long sf[4], sb[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int q0 = offsets[k], q1 = offsets[k + 1];
    long long f = 0, b = 0;
    for (int i = tid; i < ntiles; i += 256) f += fpart[(size_t)k * ntiles + i];
    for (int q = q0 + tid; q < q1; q += 256) b += (long long)colmax[q];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { f += __shfl_xor(f, d); b += __shfl_xor(b, d); }
    if ((tid & 63) == 0) { sf[tid >> 6] = f; sb[tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) { fwd[k] = sf[0] + sf[1] + sf[2] + sf[3]; bwd[k] = sb[0] + sb[1] + sb[2] + sb[3]; }
}

// a, rows, offsets ([N + 1], on the device), fwd, bwd ([N] int64): device pointers; total = offsets[N], known to the host
int nctk_descriptor_match(nct_ctx* ctx, hipStream_t s, const int8_t* a, int na, int C, const int8_t* rows, const int* offsets, int N, int total, long long* fwd, long long* bwd) {
    const int ntiles = cdiv(na, DM_TM);
    DevBuf<long long> fpart(ctx, (size_t)N * ntiles);
    DevBuf<int> colmax(ctx, (size_t)total);
    if (!fpart.ok() || !colmax.ok()) return NCT_ERR_HIP;
    NCT_HIP(hipMemsetD32Async((hipDeviceptr_t)(int*)colmax, INT_MIN, (size_t)total, s));
    hipLaunchKernelGGL(k_desc_match, dim3(ntiles, N), dim3(256), 0, s, (const signed char*)a, na, C, (const signed char*)rows, offsets, (long long*)fpart, (int*)colmax);
    NCT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_desc_sums, dim3(N), dim3(256), 0, s, (const long long*)fpart, ntiles, (const int*)colmax, offsets, fwd, bwd);
    NCT_LAUNCH_CHECK();
    return 0;
}
