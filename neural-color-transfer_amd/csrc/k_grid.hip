// k_grid.hip — local colour grids (SPEC §6.22): a bilateral grid of 3 x 4 affine BGR maps over (row, column, luma). The integer splat of a (source, result) pair onto
// the pixels' nearest nodes, the integer blur with one 4 x 4 L D L^T solve per node, and the apply on 8-bit and 16-bit pixels of any size. tests/grid_ref.py is the
// numpy form of every operation here, in the same order.
#include "nct_internal.h"

#define GRID_NSUM 22                        // 10 Gram sums (j <= k over B, G, R, 1; [9] is the count), then 12 right-hand sides [c][j]
#define GRID_MAX_GZ 32
#define GRID_TX 32                          // the apply's tile: k_finish_up's
#define GRID_TY 8
#define GRID_SLICE_PIXELS 4096              // a splat workgroup's share of a node's rectangle: 16 pixels per thread

typedef unsigned long long u64;

// ================================================================= positions (rule 2)
// row y of H under g nodes: t = (2 y + 1)(g - 1) over 2 H
__device__ __forceinline__ void grid_axis(int y, int H, int g, int& i, int& f) {
    const int t = (2 * y + 1) * (g - 1);    // below 2^15 * 63
    i = min(t / (2 * H), g - 2);
    f = t - 2 * H * i;
}
__device__ __forceinline__ int grid_luma(int b, int g, int r) { return (29 * b + 150 * g + 77 * r + 128) >> 8; }
// the first row whose nearest node is n: ceil((2 H n - H) / (g - 1)) / 2, 0 for node 0 and H behind the last node
__host__ __device__ __forceinline__ int grid_rect_lo(int n, int g, int H) {
    if (n <= 0) return 0;
    if (n >= g) return H;
    const int a = 2 * H * n - H, q = (a + g - 2) / (g - 1);
    return min(H, q / 2);
}

// ================================================================= splat (rule 3)
// The pixels whose nearest spatial node is (ny, nx) form the rectangle grid_rect_lo gives. A workgroup takes a band of rows of one node's rectangle (blockIdx.y: the
// node, blockIdx.x: the band, `rows` rows each) and sums its pixels into gz x 22 int64 words of LDS, one private copy per wave so that the lanes of different waves never
// meet on a word; the non-zero totals then go to the zeroed global accumulators with 64-bit integer atomics. Integers only: the order of the adds does not matter.
__global__ __launch_bounds__(256) void k_grid_splat(const uint8_t* __restrict__ S, const uint8_t* __restrict__ O, int H, int W, int gy, int gx, int gz, int slice_pixels,
                                                    u64* __restrict__ sums) {
    __shared__ u64 acc[4][GRID_MAX_GZ * GRID_NSUM];
    const int ny = blockIdx.y / gx, nx = blockIdx.y - ny * gx;
    const int y_lo = grid_rect_lo(ny, gy, H), y_hi = grid_rect_lo(ny + 1, gy, H);
    const int x_lo = grid_rect_lo(nx, gx, W), x_hi = grid_rect_lo(nx + 1, gx, W);
    const int rw = x_hi - x_lo;
    if (rw <= 0) return;
    const int rows = max(1, slice_pixels / rw);
    const int r0 = y_lo + (int)blockIdx.x * rows, r1 = min(r0 + rows, y_hi);
    if (r0 >= y_hi) return;                                         // uniform over the workgroup: nobody waits at a barrier
    const int nacc = gz * GRID_NSUM;
    for (int i = threadIdx.x; i < 4 * GRID_MAX_GZ * GRID_NSUM; i += 256) (&acc[0][0])[i] = 0ull;
    __syncthreads();
    u64* mine = acc[threadIdx.x >> 6];
    const int cnt = (r1 - r0) * rw;
    for (int p = threadIdx.x; p < cnt; p += 256) {
        const int y = r0 + p / rw, x = x_lo + p % rw;
        const size_t at = ((size_t)y * W + x) * 3;
        long long s[4], d[3];
        for (int c = 0; c < 3; ++c) { s[c] = (long long)S[at + c]; d[c] = (long long)O[at + c] - s[c]; }
        s[3] = 1;
        const int tz = grid_luma((int)s[0], (int)s[1], (int)s[2]) * (gz - 1);
        u64* a = mine + ((2 * tz + 255) / 510) * GRID_NSUM;         // the nearest luma node
        int k = 0;
        for (int j = 0; j < 4; ++j) for (int l = j; l < 4; ++l, ++k) { const long long v = s[j] * s[l]; if (v) atomicAdd(a + k, (u64)v); }
        for (int c = 0; c < 3; ++c) for (int j = 0; j < 4; ++j, ++k) { const long long v = s[j] * d[c]; if (v) atomicAdd(a + k, (u64)v); }
    }
    __syncthreads();
    u64* dst = sums + (size_t)blockIdx.y * gz * GRID_NSUM;
    for (int i = threadIdx.x; i < nacc; i += 256) {
        const u64 v = acc[0][i] + acc[1][i] + acc[2][i] + acc[3][i];
        if (v) atomicAdd(dst + i, v);
    }
}

// ================================================================= blur and solve (rules 4 and 5): one thread per node
__global__ __launch_bounds__(256) void k_grid_solve(const long long* __restrict__ sums, int gy, int gx, int gz, double lam, long long* __restrict__ blurred, double* __restrict__ X) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= gy * gx * gz) return;
    const int z = n % gz, x = (n / gz) % gx, y = n / (gz * gx);
    long long b[GRID_NSUM];
    for (int k = 0; k < GRID_NSUM; ++k) b[k] = 0;
    for (int dy = -1; dy <= 1; ++dy) { if (y + dy < 0 || y + dy >= gy) continue;
    for (int dx = -1; dx <= 1; ++dx) { if (x + dx < 0 || x + dx >= gx) continue;
    for (int dz = -1; dz <= 1; ++dz) { if (z + dz < 0 || z + dz >= gz) continue;
        const long long w = (dy ? 1 : 2) * (dx ? 1 : 2) * (dz ? 1 : 2);
        const long long* s = sums + (size_t)(((y + dy) * gx + x + dx) * gz + z + dz) * GRID_NSUM;
        for (int k = 0; k < GRID_NSUM; ++k) b[k] += w * s[k];
    }}}
    for (int k = 0; k < GRID_NSUM; ++k) blurred[(size_t)n * GRID_NSUM + k] = b[k];
    double* out = X + (size_t)n * 12;
    if (b[9] <= 0) { for (int k = 0; k < 12; ++k) out[k] = 0.0; return; }
    double M[4][4], L[4][4], d[4];
    { int k = 0; for (int j = 0; j < 4; ++j) for (int l = j; l < 4; ++l, ++k) M[j][l] = M[l][j] = (double)b[k]; }
    const double ridge = lam * (double)b[9];
    for (int j = 0; j < 3; ++j) M[j][j] = M[j][j] + ridge;
    for (int j = 0; j < 4; ++j) {
        double dj = M[j][j];
        for (int k = 0; k < j; ++k) dj = dj - (L[j][k] * L[j][k]) * d[k];
        d[j] = dj;
        for (int i = j + 1; i < 4; ++i) {
            double v = M[i][j];
            for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * d[k];
            L[i][j] = v / dj;
        }
    }
    for (int c = 0; c < 3; ++c) {
        double xs[4];
        for (int i = 0; i < 4; ++i) { double v = (double)b[10 + 4 * c + i]; for (int k = 0; k < i; ++k) v = v - L[i][k] * xs[k]; xs[i] = v; }
        for (int i = 0; i < 4; ++i) xs[i] = xs[i] / d[i];
        for (int i = 3; i >= 0; --i) { double v = xs[i]; for (int k = i + 1; k < 4; ++k) v = v - L[k][i] * xs[k]; xs[i] = v; }
        for (int i = 0; i < 4; ++i) out[4 * c + i] = xs[i];
    }
}

// ================================================================= apply (rule 6)
// One pixel per thread on k_finish_up's 32 x 8 tile; T in and T out, no intermediate image. The tile's pixels go through LDS both ways: as 4-byte words where the
// pointers and the row pitch allow (tile rows start on multiples of 32 pixels, so 96 or 192 bytes in), element by element otherwise and on the right edge; a tile reads
// all of its input before it writes, so out may be in. IN_LDS: a tile crosses at most one cell boundary per axis (the launcher checks 7 (gy - 1) <= H and
// 31 (gx - 1) <= W), so it touches at most 3 x 3 spatial nodes, whose gz x 12 coefficients are staged in LDS (27 KB at gz = 32; 2 x 2 nodes, 12 KB, where no
// boundary is crossed). A denser grid over a small picture reads the coefficients through L2.
template <typename T> struct grid_px;
template <> struct grid_px<uint8_t> { static constexpr int Z = 255; static constexpr double K = 1.0; };
template <> struct grid_px<uint16_t> { static constexpr int Z = 65535; static constexpr double K = 257.0; };

template <typename T, bool IN_LDS>
__global__ __launch_bounds__(GRID_TX * GRID_TY) void k_grid_apply(const double* __restrict__ X, int gy, int gx, int gz, const T* in, int H, int W, int packed, T* out) {
    constexpr int Z = grid_px<T>::Z;
    constexpr int ROW_WORDS = GRID_TX * 3 * (int)sizeof(T) / 4;     // 24 or 48
    __shared__ double sx[IN_LDS ? 9 * GRID_MAX_GZ * 12 : 1];
    __shared__ uint32_t tile[GRID_TY * ROW_WORDS];
    T* px = (T*)tile;
    const int tid = threadIdx.y * GRID_TX + threadIdx.x;
    const int x0 = blockIdx.x * GRID_TX, y0 = blockIdx.y * GRID_TY;
    const int tw = min(GRID_TX, W - x0), th = min(GRID_TY, H - y0);
    const bool words = packed && tw == GRID_TX;
    if (words) {
        for (int i = tid; i < th * ROW_WORDS; i += GRID_TX * GRID_TY) {
            const int r = i / ROW_WORDS, k = i - r * ROW_WORDS;
            tile[i] = ((const uint32_t*)(in + ((size_t)(y0 + r) * W + x0) * 3))[k];
        }
    } else {
        for (int i = tid; i < th * tw * 3; i += GRID_TX * GRID_TY) {
            const int r = i / (tw * 3), k = i - r * tw * 3;
            px[r * GRID_TX * 3 + k] = in[((size_t)(y0 + r) * W + x0) * 3 + k];
        }
    }
    int cy0, cx0, f;
    grid_axis(y0, H, gy, cy0, f);
    grid_axis(x0, W, gx, cx0, f);
    int nnx = 2;
    if (IN_LDS) {
        int cy1, cx1;
        grid_axis(y0 + th - 1, H, gy, cy1, f);
        grid_axis(x0 + tw - 1, W, gx, cx1, f);
        const int nny = cy1 - cy0 + 2;                              // 2 or 3
        nnx = cx1 - cx0 + 2;
        const int per = gz * 12;
        for (int i = tid; i < nny * nnx * per; i += GRID_TX * GRID_TY) {
            const int sn = i / per, k = i - sn * per;
            const int yy = sn / nnx, xx = sn - yy * nnx;
            sx[i] = X[(size_t)((cy0 + yy) * gx + cx0 + xx) * per + k];
        }
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool inside = x < W && y < H;
    unsigned res[3] = {0u, 0u, 0u};
    if (inside) {
        const T* p = px + (threadIdx.y * GRID_TX + threadIdx.x) * 3;
        const int sb = (int)p[0], sg = (int)p[1], sr = (int)p[2];
        int iy, fy, ix, fx;
        grid_axis(y, H, gy, iy, fy);
        grid_axis(x, W, gx, ix, fx);
        const int tz = grid_luma(sb, sg, sr) * (gz - 1);
        const int iz = min(tz / Z, gz - 2), fz = tz - Z * iz;
        double acc[12];
        for (int k = 0; k < 12; ++k) acc[k] = 0.0;
        for (int dy = 0; dy < 2; ++dy) {
            const u64 wy = (u64)(dy ? fy : 2 * H - fy);
            for (int dx = 0; dx < 2; ++dx) {
                const u64 wyx = wy * (u64)(dx ? fx : 2 * W - fx);
                const double* base = IN_LDS ? sx + (size_t)(((iy + dy - cy0) * nnx + ix + dx - cx0) * gz + iz) * 12
                                            : X + ((size_t)((iy + dy) * gx + ix + dx) * gz + iz) * 12;
                for (int dz = 0; dz < 2; ++dz) {
                    const double w = (double)(wyx * (u64)(dz ? fz : Z - fz));       // at most 2^46: exact
                    for (int k = 0; k < 12; ++k) acc[k] += w * base[12 * dz + k];
                }
            }
        }
        const double Dn = ((double)(2 * H) * (double)(2 * W)) * (double)Z;
        const double s[3] = {(double)sb, (double)sg, (double)sr};
        for (int c = 0; c < 3; ++c) {
            const double t = ((acc[4 * c] * s[0] + acc[4 * c + 1] * s[1]) + acc[4 * c + 2] * s[2]) + acc[4 * c + 3] * grid_px<T>::K;
            double v = s[c] + t / Dn;
            v = v > 0.0 ? v : 0.0; v = v < (double)Z ? v : (double)Z;               // A1's cast: a NaN becomes 0; clamp, then round to nearest even
            res[c] = (unsigned)(int)rint(v);
        }
    }
    __syncthreads();                                                // every thread has read its pixel: the tile now takes the outputs
    if (inside) { T* q = px + (threadIdx.y * GRID_TX + threadIdx.x) * 3; q[0] = (T)res[0]; q[1] = (T)res[1]; q[2] = (T)res[2]; }
    __syncthreads();
    if (words) {
        for (int i = tid; i < th * ROW_WORDS; i += GRID_TX * GRID_TY) {
            const int r = i / ROW_WORDS, k = i - r * ROW_WORDS;
            ((uint32_t*)(out + ((size_t)(y0 + r) * W + x0) * 3))[k] = tile[i];
        }
    } else {
        for (int i = tid; i < th * tw * 3; i += GRID_TX * GRID_TY) {
            const int r = i / (tw * 3), k = i - r * tw * 3;
            out[((size_t)(y0 + r) * W + x0) * 3 + k] = px[r * GRID_TX * 3 + k];
        }
    }
}

// ================================================================= launchers
int nctk_grid_splat(nct_ctx* ctx, hipStream_t s, const uint8_t* src, const uint8_t* res, int H, int W, int gy, int gx, int gz, int64_t* sums) {
    // the arena clears nothing: the accumulators are zeroed on the stream in front of the splat
    NCT_HIP(hipMemsetAsync(sums, 0, (size_t)gy * gx * gz * GRID_NSUM * sizeof(int64_t), s));
    // the bands of the largest rectangle decide the grid; a node with fewer bands leaves its surplus workgroups at once
    int bands = 1;
    for (int ny = 0; ny < gy; ++ny) for (int nx = 0; nx < gx; ++nx) {
        const int rh = grid_rect_lo(ny + 1, gy, H) - grid_rect_lo(ny, gy, H), rw = grid_rect_lo(nx + 1, gx, W) - grid_rect_lo(nx, gx, W);
        if (rh <= 0 || rw <= 0) continue;
        const int rows = std::max(1, GRID_SLICE_PIXELS / rw);
        bands = std::max(bands, cdiv(rh, rows));
    }
    k_grid_splat<<<dim3(bands, gy * gx), 256, 0, s>>>(src, res, H, W, gy, gx, gz, GRID_SLICE_PIXELS, (u64*)sums);
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}

int nctk_grid_solve(nct_ctx* ctx, hipStream_t s, const int64_t* sums, int gy, int gx, int gz, double lambda, int64_t* blurred, double* X) {
    k_grid_solve<<<cdiv(gy * gx * gz, 256), 256, 0, s>>>((const long long*)sums, gy, gx, gz, lambda, (long long*)blurred, X);
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}

template <typename T>
static int grid_apply_launch(nct_ctx* ctx, hipStream_t s, const double* X, int gy, int gx, int gz, const T* in, int H, int W, T* out) {
    const dim3 grid(cdiv(W, GRID_TX), cdiv(H, GRID_TY)), block(GRID_TX, GRID_TY);
    // word access: both bases on 4 bytes and every row's pitch a multiple of 4 bytes
    const int packed = (((uintptr_t)in | (uintptr_t)out) & 3) == 0 && ((size_t)W * 3 * sizeof(T)) % 4 == 0;
    if ((GRID_TY - 1) * (gy - 1) <= H && (GRID_TX - 1) * (gx - 1) <= W) k_grid_apply<T, true><<<grid, block, 0, s>>>(X, gy, gx, gz, in, H, W, packed, out);
    else k_grid_apply<T, false><<<grid, block, 0, s>>>(X, gy, gx, gz, in, H, W, packed, out);
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}
int nctk_grid_apply(nct_ctx* ctx, hipStream_t s, const double* X, int gy, int gx, int gz, const uint8_t* in, int H, int W, uint8_t* out) {
    return grid_apply_launch<uint8_t>(ctx, s, X, gy, gx, gz, in, H, W, out);
}
int nctk_grid_apply16(nct_ctx* ctx, hipStream_t s, const double* X, int gy, int gx, int gz, const uint16_t* in, int H, int W, uint16_t* out) {
    return grid_apply_launch<uint16_t>(ctx, s, X, gy, gx, gz, in, H, W, out);
}
