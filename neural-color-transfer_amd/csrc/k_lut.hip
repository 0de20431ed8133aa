// k_lut.hip — 3D colour look-up tables (SPEC §6.6): the integer splat of a (source, result) pair onto an N^3 lattice, the multigrid solve of the
// displacement field, the table, and the trilinear apply. tests/lut_ref.py is the numpy form of every operation here, in the same order. The apply on 16-bit pixels
// (SPEC §6.20): tests/lut16_ref.py.
#include "nct_internal.h"

#define LUT_W3 16581375.0                   // 255^3: the sum of a pixel's eight integer weights
#define LUT_HASH 1024                       // slots of the splat's workgroup-private accumulator
#define LUT_PROBES 8
#define LUT_MAXLEV 6                        // 65 -> 33 -> 17 -> 9 -> 5 -> 3
#define LUT_TAIL_N 9                        // lattices up to this size run inside one workgroup, larger ones one launch per operation

typedef unsigned long long u64;

// ================================================================= lattice coordinates of an 8-bit value (rule 2)
__device__ __forceinline__ void lut_axis(int v, int N, int& i, int& f) {
    const int t = v * (N - 1);
    i = min(t / 255, N - 2);
    f = t - 255 * i;
}

// pixels p0 .. p0 + 3 of a tightly packed 3-byte image as three words (base 4-byte aligned, p0 a multiple of 4), else byte by byte; cnt <= 4 pixels are valid
__device__ __forceinline__ void lut_load4(const uint8_t* __restrict__ img, long p0, int cnt, bool packed, uint32_t w[3]) {
    if (packed && cnt == 4) {
        const uint32_t* q = (const uint32_t*)(img + p0 * 3);
        w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
    } else {
        w[0] = w[1] = w[2] = 0u;
        for (int k = 0; k < cnt * 3; ++k) w[k >> 2] |= (uint32_t)img[p0 * 3 + k] << (8 * (k & 3));
    }
}
__device__ __forceinline__ int lut_byte(const uint32_t w[3], int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// ================================================================= splat (rule 3)
// A scatter with heavy contention: a photograph puts most of its pixels into a few hundred cells. Every workgroup sums its contiguous run of pixels into an LDS hash of
// lattice nodes (64-bit integer LDS atomics: weight and three residual sums per slot) and adds each occupied slot to the global accumulators once at the end: four consecutive
// lanes add a node's weight (8 B of W) and its three residuals (24 contiguous bytes of R). A node that finds no slot within LUT_PROBES steps goes to the global accumulators directly. Integer sums: the order of the adds does not matter.
__device__ __forceinline__ int lut_slot(int* keys, int node) {
    unsigned h = ((unsigned)node * 2654435761u) >> 22;
    for (int p = 0; p < LUT_PROBES; ++p) {
        const int k = atomicCAS(&keys[h], -1, node);
        if (k == -1 || k == node) return (int)h;
        h = (h + 1) & (LUT_HASH - 1);
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_lut_splat(const uint8_t* __restrict__ S, const uint8_t* __restrict__ O, long npix, long chunk, int N, int packed,
                                                   u64* __restrict__ W, u64* __restrict__ R) {
    __shared__ int keys[LUT_HASH];
    __shared__ u64 acc[LUT_HASH * 4];
    for (int i = threadIdx.x; i < LUT_HASH; i += 256) keys[i] = -1;
    for (int i = threadIdx.x; i < LUT_HASH * 4; i += 256) acc[i] = 0ull;
    __syncthreads();
    const long first = (long)blockIdx.x * chunk, last = min(first + chunk, npix);          // chunk is a multiple of 4
    for (long p0 = first + (long)threadIdx.x * 4; p0 < last; p0 += 256 * 4) {
        const int cnt = (int)min(4L, last - p0);
        uint32_t sw[3], ow[3];
        lut_load4(S, p0, cnt, packed != 0, sw);
        lut_load4(O, p0, cnt, packed != 0, ow);
        for (int j = 0; j < cnt; ++j) {
            int ib, fb, ig, fg, ir, fr;
            lut_axis(lut_byte(sw, 3 * j), N, ib, fb); lut_axis(lut_byte(sw, 3 * j + 1), N, ig, fg); lut_axis(lut_byte(sw, 3 * j + 2), N, ir, fr);
            long long d[3];
            for (int c = 0; c < 3; ++c) d[c] = (long long)(lut_byte(ow, 3 * j + c) - lut_byte(sw, 3 * j + c));
            for (int corner = 0; corner < 8; ++corner) {
                const int db = corner >> 2, dg = (corner >> 1) & 1, dr = corner & 1;
                const long long w = (long long)((db ? fb : 255 - fb) * (dg ? fg : 255 - fg)) * (long long)(dr ? fr : 255 - fr);
                if (w == 0) continue;
                const int node = ((ib + db) * N + ig + dg) * N + ir + dr;
                const int slot = lut_slot(keys, node);
                u64* dst = slot >= 0 ? &acc[slot * 4] : nullptr;
                if (dst) atomicAdd(dst, (u64)w); else atomicAdd(&W[node], (u64)w);
                for (int c = 0; c < 3; ++c) {
                    if (d[c] == 0) continue;
                    if (dst) atomicAdd(dst + 1 + c, (u64)(w * d[c])); else atomicAdd(&R[(size_t)node * 3 + c], (u64)(w * d[c]));
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LUT_HASH * 4; i += 256) {
        const int key = keys[i >> 2], comp = i & 3;
        const u64 v = acc[i];
        if (key < 0 || v == 0ull) continue;
        if (comp == 0) atomicAdd(&W[key], v); else atomicAdd(&R[(size_t)key * 3 + comp - 1], v);
    }
}

// The masked splat (SPEC §6.11 rule 7): k_lut_splat over the pixels with M >= 128 only, a kernel of its own so that the unmasked one stays as it is. The integer sums
// are order-free, so it equals the splat of the subsequence of kept pixels. kept: the number of kept pixels, one atomic per workgroup (zeroed by the launcher).
__global__ __launch_bounds__(256) void k_lut_splat_masked(const uint8_t* __restrict__ S, const uint8_t* __restrict__ O, const uint8_t* __restrict__ M, long npix, long chunk, int N,
                                                          int packed, u64* __restrict__ W, u64* __restrict__ R, u64* __restrict__ kept) {
    __shared__ int keys[LUT_HASH];
    __shared__ u64 acc[LUT_HASH * 4];
    __shared__ unsigned nkept;
    for (int i = threadIdx.x; i < LUT_HASH; i += 256) keys[i] = -1;
    for (int i = threadIdx.x; i < LUT_HASH * 4; i += 256) acc[i] = 0ull;
    if (threadIdx.x == 0) nkept = 0u;
    __syncthreads();
    const long first = (long)blockIdx.x * chunk, last = min(first + chunk, npix);          // chunk is a multiple of 4
    unsigned mine = 0u;
    for (long p0 = first + (long)threadIdx.x * 4; p0 < last; p0 += 256 * 4) {
        const int cnt = (int)min(4L, last - p0);
        uint32_t sw[3], ow[3];
        lut_load4(S, p0, cnt, packed != 0, sw);
        lut_load4(O, p0, cnt, packed != 0, ow);
        for (int j = 0; j < cnt; ++j) {
            if (M[p0 + j] < 128) continue;
            ++mine;
            int ib, fb, ig, fg, ir, fr;
            lut_axis(lut_byte(sw, 3 * j), N, ib, fb); lut_axis(lut_byte(sw, 3 * j + 1), N, ig, fg); lut_axis(lut_byte(sw, 3 * j + 2), N, ir, fr);
            long long d[3];
            for (int c = 0; c < 3; ++c) d[c] = (long long)(lut_byte(ow, 3 * j + c) - lut_byte(sw, 3 * j + c));
            for (int corner = 0; corner < 8; ++corner) {
                const int db = corner >> 2, dg = (corner >> 1) & 1, dr = corner & 1;
                const long long w = (long long)((db ? fb : 255 - fb) * (dg ? fg : 255 - fg)) * (long long)(dr ? fr : 255 - fr);
                if (w == 0) continue;
                const int node = ((ib + db) * N + ig + dg) * N + ir + dr;
                const int slot = lut_slot(keys, node);
                u64* dst = slot >= 0 ? &acc[slot * 4] : nullptr;
                if (dst) atomicAdd(dst, (u64)w); else atomicAdd(&W[node], (u64)w);
                for (int c = 0; c < 3; ++c) {
                    if (d[c] == 0) continue;
                    if (dst) atomicAdd(dst + 1 + c, (u64)(w * d[c])); else atomicAdd(&R[(size_t)node * 3 + c], (u64)(w * d[c]));
                }
            }
        }
    }
    if (mine) atomicAdd(&nkept, mine);
    __syncthreads();
    for (int i = threadIdx.x; i < LUT_HASH * 4; i += 256) {
        const int key = keys[i >> 2], comp = i & 3;
        const u64 v = acc[i];
        if (key < 0 || v == 0ull) continue;
        if (comp == 0) atomicAdd(&W[key], v); else atomicAdd(&R[(size_t)key * 3 + comp - 1], v);
    }
    if (threadIdx.x == 0 && nkept) atomicAdd(kept, (u64)nkept);
}

// ================================================================= solve (rules 4-7): element-wise operations, each over `count` elements from `tid` in steps of `nth`
// A level's operator is a 27-point stencil A [n^3][27], entry e = (db + 1) * 9 + (dg + 1) * 3 + dr + 1; an entry whose neighbour lies outside the lattice is 0.0.
struct lut_level { int n; double* A; double* q; double* x; double* t; double* b; double* r; };
struct lut_hier { int nlev; lut_level lv[LUT_MAXLEV]; double* ldl; /* [27 * 27 + 27] L, d of the coarsest operator */ };

__device__ void lut_op_fine(const u64* __restrict__ W, const long long* __restrict__ R, double lam, const lut_level& l, int tid, int nth) {
    const int n = l.n, n3 = n * n * n;
    for (int i = tid; i < n3; i += nth) {
        const int z = i / (n * n), y = (i / n) % n, x = i % n;
        const double deg = (double)((z > 0) + (z < n - 1) + (y > 0) + (y < n - 1) + (x > 0) + (x < n - 1));
        double* a = l.A + (size_t)i * 27;
        for (int e = 0; e < 27; ++e) a[e] = 0.0;
        a[13] = (double)W[i] / LUT_W3 + lam * deg;
        if (z > 0) a[4] = -lam;
        if (y > 0) a[10] = -lam;
        if (x > 0) a[12] = -lam;
        if (x < n - 1) a[14] = -lam;
        if (y < n - 1) a[16] = -lam;
        if (z < n - 1) a[22] = -lam;
        for (int c = 0; c < 3; ++c) { l.b[(size_t)i * 3 + c] = (double)R[(size_t)i * 3 + c] / LUT_W3; l.x[(size_t)i * 3 + c] = 0.0; }
    }
}

// P^T A P: coarse entry (I, delta) = sum over a (outer) and e (inner) of P(a) P(b) A[2 I + a, e], b = a + e - 2 delta inside {-1, 0, 1}^3, P(a) = 2^-|a|_1
__device__ void lut_op_galerkin(const lut_level& f, const lut_level& c, int tid, int nth) {
    const int n = f.n, m = c.n, cnt = m * m * m * 27;
    for (int i = tid; i < cnt; i += nth) {
        const int k = i % 27, I = i / 27;
        const int Z = I / (m * m), Y = (I / m) % m, X = I % m;
        const int kz = k / 9 - 1, ky = (k / 3) % 3 - 1, kx = k % 3 - 1;
        double acc = 0.0;
        for (int az = -1; az <= 1; ++az) { const int z = 2 * Z + az; if (z < 0 || z >= n) continue;
        for (int ay = -1; ay <= 1; ++ay) { const int y = 2 * Y + ay; if (y < 0 || y >= n) continue;
        for (int ax = -1; ax <= 1; ++ax) { const int x = 2 * X + ax; if (x < 0 || x >= n) continue;
            const double* a = f.A + ((size_t)(z * n + y) * n + x) * 27;
            const double wa = (az ? 0.5 : 1.0) * (ay ? 0.5 : 1.0) * (ax ? 0.5 : 1.0);
            for (int ez = -1; ez <= 1; ++ez) { const int bz = az + ez - 2 * kz; if (bz < -1 || bz > 1) continue;
            for (int ey = -1; ey <= 1; ++ey) { const int by = ay + ey - 2 * ky; if (by < -1 || by > 1) continue;
            for (int ex = -1; ex <= 1; ++ex) { const int bx = ax + ex - 2 * kx; if (bx < -1 || bx > 1) continue;
                const double w = wa * ((bz ? 0.5 : 1.0) * (by ? 0.5 : 1.0) * (bx ? 0.5 : 1.0));
                acc += w * a[(ez + 1) * 9 + (ey + 1) * 3 + ex + 1];
            }}}
        }}}
        c.A[i] = acc;
    }
}

// the smoother's divisor q = max(1.25 A_ii, 0.625 sum_e |A_ie|)
__device__ void lut_op_divisor(const lut_level& l, int tid, int nth) {
    const int n3 = l.n * l.n * l.n;
    for (int i = tid; i < n3; i += nth) {
        const double* a = l.A + (size_t)i * 27;
        double l1 = 0.0;
        for (int e = 0; e < 27; ++e) l1 += fabs(a[e]);
        l.q[i] = fmax(1.25 * a[13], 0.625 * l1);
    }
}

// A x at element (node i, channel c): the 27 taps in stencil order, those outside the lattice skipped
__device__ __forceinline__ double lut_row(const lut_level& l, const double* __restrict__ x, int i, int c) {
    const int n = l.n;
    const int z = i / (n * n), y = (i / n) % n, xx = i % n;
    const double* a = l.A + (size_t)i * 27;
    double acc = 0.0;
    for (int dz = -1; dz <= 1; ++dz) { if (z + dz < 0 || z + dz >= n) continue;
    for (int dy = -1; dy <= 1; ++dy) { if (y + dy < 0 || y + dy >= n) continue;
    for (int dx = -1; dx <= 1; ++dx) { if (xx + dx < 0 || xx + dx >= n) continue;
        acc += a[(dz + 1) * 9 + (dy + 1) * 3 + dx + 1] * x[(size_t)(i + (dz * n + dy) * n + dx) * 3 + c];
    }}}
    return acc;
}
// one smoothing step, out of place: out = x + (b - A x) / q
__device__ void lut_op_smooth(const lut_level& l, const double* __restrict__ x, double* __restrict__ out, int tid, int nth) {
    const int cnt = l.n * l.n * l.n * 3;
    for (int j = tid; j < cnt; j += nth) { const int i = j / 3, c = j - 3 * i; out[j] = x[j] + (l.b[j] - lut_row(l, x, i, c)) / l.q[i]; }
}
__device__ void lut_op_residual(const lut_level& l, int tid, int nth) {
    const int cnt = l.n * l.n * l.n * 3;
    for (int j = tid; j < cnt; j += nth) { const int i = j / 3, c = j - 3 * i; l.r[j] = l.b[j] - lut_row(l, l.x, i, c); }
}
// coarse right-hand side = P^T r (full weighting, no scaling), taps db outer, dr inner, those outside skipped; the coarse correction starts at zero
__device__ void lut_op_restrict(const lut_level& f, const lut_level& c, int tid, int nth) {
    const int n = f.n, m = c.n, cnt = m * m * m * 3;
    for (int j = tid; j < cnt; j += nth) {
        const int I = j / 3, ch = j - 3 * I;
        const int Z = I / (m * m), Y = (I / m) % m, X = I % m;
        double acc = 0.0;
        for (int dz = -1; dz <= 1; ++dz) { const int z = 2 * Z + dz; if (z < 0 || z >= n) continue;
        for (int dy = -1; dy <= 1; ++dy) { const int y = 2 * Y + dy; if (y < 0 || y >= n) continue;
        for (int dx = -1; dx <= 1; ++dx) { const int x = 2 * X + dx; if (x < 0 || x >= n) continue;
            acc += ((dz ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0)) * f.r[((size_t)(z * n + y) * n + x) * 3 + ch];
        }}}
        c.b[j] = acc; c.x[j] = 0.0;
    }
}
// x += P x_coarse: per axis an even node copies its coarse node, an odd one takes half of each neighbour, taps b outer, r inner
__device__ void lut_op_prolong_add(const lut_level& f, const lut_level& c, int tid, int nth) {
    const int n = f.n, m = c.n, cnt = n * n * n * 3;
    for (int j = tid; j < cnt; j += nth) {
        const int i = j / 3, ch = j - 3 * i;
        const int z = i / (n * n), y = (i / n) % n, x = i % n;
        double acc = 0.0;
        for (int tz = 0; tz <= (z & 1); ++tz) for (int ty = 0; ty <= (y & 1); ++ty) for (int tx = 0; tx <= (x & 1); ++tx) {
            const double w = ((z & 1) ? 0.5 : 1.0) * ((y & 1) ? 0.5 : 1.0) * ((x & 1) ? 0.5 : 1.0);
            acc += w * c.x[((size_t)(((z >> 1) + tz) * m + (y >> 1) + ty) * m + (x >> 1) + tx) * 3 + ch];
        }
        f.x[j] = f.x[j] + acc;
    }
}
// the coarsest lattice (27 nodes): its stencil, with 0.0 between nodes two apart on an axis, is the dense matrix; L D L^T by one thread, rows and sums in ascending order
__device__ void lut_ldl_factor(const lut_level& l, double* __restrict__ ldl) {
    double* L = ldl; double* d = ldl + 27 * 27;
    for (int j = 0; j < 27; ++j) {
        const int jz = j / 9, jy = (j / 3) % 3, jx = j % 3;
        double dj = l.A[(size_t)j * 27 + 13];
        for (int k = 0; k < j; ++k) dj = dj - (L[j * 27 + k] * L[j * 27 + k]) * d[k];
        d[j] = dj;
        for (int i = j + 1; i < 27; ++i) {
            // A[i][j]: the stencil entry of row i that points at node j; nodes two apart on an axis are not coupled
            const int dz = jz - i / 9, dy = jy - (i / 3) % 3, dx = jx - i % 3;
            double v = (dz < -1 || dy < -1 || dy > 1 || dx < -1 || dx > 1) ? 0.0 : l.A[(size_t)i * 27 + (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)];
            for (int k = 0; k < j; ++k) v = v - (L[i * 27 + k] * L[j * 27 + k]) * d[k];
            L[i * 27 + j] = v / dj;
        }
    }
}
// x = A^-1 b of the coarsest level for channel c (one thread per channel)
__device__ void lut_ldl_solve(const lut_level& l, const double* __restrict__ ldl, int c) {
    const double* L = ldl; const double* d = ldl + 27 * 27;
    double* x = l.x + c;                                       // x_i lives at x[3 i]
    for (int i = 0; i < 27; ++i) { double v = l.b[i * 3 + c]; for (int k = 0; k < i; ++k) v = v - L[i * 27 + k] * x[3 * k]; x[3 * i] = v; }
    for (int i = 0; i < 27; ++i) x[3 * i] = x[3 * i] / d[i];
    for (int i = 26; i >= 0; --i) { double v = x[3 * i]; for (int k = i + 1; k < 27; ++k) v = v - L[k * 27 + i] * x[3 * k]; x[3 * i] = v; }
}

// ---- the operations as launches of their own: the levels above LUT_TAIL_N^3
#define LUT_GRID_ARGS (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x)
__global__ void k_lut_fine(const u64* W, const long long* R, double lam, lut_level l) { lut_op_fine(W, R, lam, l, LUT_GRID_ARGS); }
__global__ void k_lut_galerkin(lut_level f, lut_level c) { lut_op_galerkin(f, c, LUT_GRID_ARGS); }
__global__ void k_lut_divisor(lut_level l) { lut_op_divisor(l, LUT_GRID_ARGS); }
__global__ void k_lut_smooth(lut_level l, const double* x, double* out) { lut_op_smooth(l, x, out, LUT_GRID_ARGS); }
__global__ void k_lut_residual(lut_level l) { lut_op_residual(l, LUT_GRID_ARGS); }
__global__ void k_lut_restrict(lut_level f, lut_level c) { lut_op_restrict(f, c, LUT_GRID_ARGS); }
__global__ void k_lut_prolong_add(lut_level f, lut_level c) { lut_op_prolong_add(f, c, LUT_GRID_ARGS); }

// ---- one workgroup: everything from level k0 (the first of at most LUT_TAIL_N^3 nodes) down. A launch per operation would leave these small lattices waiting on launch
// latency alone (DESIGN.md §9 lesson (ii)); inside one workgroup a barrier orders the operations. 17^3 does not belong here: one compute unit needs 713 us for a
// cycle from 17^3 down, a launch per operation over the whole chip about 9 us per operation.
__global__ __launch_bounds__(1024) void k_lut_tail_setup(lut_hier h, int k0) {
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int k = k0; k < h.nlev; ++k) {
        if (k > k0) { lut_op_galerkin(h.lv[k - 1], h.lv[k], tid, nth); __syncthreads(); }
        lut_op_divisor(h.lv[k], tid, nth);
    }
    __syncthreads();
    if (tid == 0) lut_ldl_factor(h.lv[h.nlev - 1], h.ldl);
}
// `cycles` V(2,2) cycles of levels k0 .. nlev - 1 on level k0's x and b (from a launch above: one cycle, x zeroed by the restriction)
__global__ __launch_bounds__(1024) void k_lut_tail_cycle(lut_hier h, int k0, int cycles) {
    const int tid = threadIdx.x, nth = blockDim.x, last = h.nlev - 1;
    for (int it = 0; it < cycles; ++it) {
        for (int k = k0; k < last; ++k) {
            const lut_level& l = h.lv[k];
            lut_op_smooth(l, l.x, l.t, tid, nth); __syncthreads();
            lut_op_smooth(l, l.t, l.x, tid, nth); __syncthreads();
            lut_op_residual(l, tid, nth); __syncthreads();
            lut_op_restrict(l, h.lv[k + 1], tid, nth); __syncthreads();
        }
        if (tid < 3) lut_ldl_solve(h.lv[last], h.ldl, tid);
        __syncthreads();
        for (int k = last - 1; k >= k0; --k) {
            const lut_level& l = h.lv[k];
            lut_op_prolong_add(l, h.lv[k + 1], tid, nth); __syncthreads();
            lut_op_smooth(l, l.x, l.t, tid, nth); __syncthreads();
            lut_op_smooth(l, l.t, l.x, tid, nth); __syncthreads();
        }
    }
}

// table (rule 8): LUT_n[c] = (float)(255 i_c / (N - 1) + D_n[c]), channels BGR = node index [ib][ig][ir]
__global__ void k_lut_table(const double* __restrict__ D, int N, float* __restrict__ lut) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N * N * N * 3) return;
    const int i = j / 3, c = j - 3 * i;
    const int idx = c == 0 ? i / (N * N) : (c == 1 ? (i / N) % N : i % N);
    lut[j] = (float)(((double)idx * 255.0) / (double)(N - 1) + D[j]);
}

// ================================================================= apply (rule 9)
// 3 B in and 3 B out per pixel, four pixels (three words) per thread. A table of up to 17^3 nodes (59 KB) is copied to LDS by every workgroup, which then walks
// many groups of pixels; larger tables (431 KB, 3.3 MB) are read through L2.
#define LUT_LDS_FLOATS (17 * 17 * 17 * 3)
template <bool IN_LDS>
__global__ __launch_bounds__(256) void k_lut_apply(const float* __restrict__ lut, int N, const uint8_t* in, long npix, int packed, uint8_t* out) {   // out may be in
    __shared__ float sl[IN_LDS ? LUT_LDS_FLOATS : 1];
    const float* tab = lut;
    if (IN_LDS) {
        for (int i = threadIdx.x; i < N * N * N * 3; i += 256) sl[i] = lut[i];
        __syncthreads();
        tab = sl;
    }
    const long groups = (npix + 3) / 4;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long p0 = g * 4;
        const int cnt = (int)min(4L, npix - p0);
        uint32_t w[3], o[3] = {0u, 0u, 0u};
        lut_load4(in, p0, cnt, packed != 0, w);
        for (int j = 0; j < cnt; ++j) {
            int ib, fb, ig, fg, ir, fr;
            lut_axis(lut_byte(w, 3 * j), N, ib, fb); lut_axis(lut_byte(w, 3 * j + 1), N, ig, fg); lut_axis(lut_byte(w, 3 * j + 2), N, ir, fr);
            double acc[3] = {0.0, 0.0, 0.0};
            for (int corner = 0; corner < 8; ++corner) {
                const int db = corner >> 2, dg = (corner >> 1) & 1, dr = corner & 1;
                const double wt = (double)((db ? fb : 255 - fb) * (dg ? fg : 255 - fg) * (dr ? fr : 255 - fr));
                const float* t = tab + (size_t)(((ib + db) * N + ig + dg) * N + ir + dr) * 3;
                for (int c = 0; c < 3; ++c) acc[c] += wt * (double)t[c];
            }
            for (int c = 0; c < 3; ++c) {
                double v = acc[c] / LUT_W3;
                v = v > 0.0 ? v : 0.0; v = v < 255.0 ? v : 255.0;                       // A1's cast: clamp, then round to nearest even
                const int k = 3 * j + c;
                o[k >> 2] |= (uint32_t)(int)rint(v) << (8 * (k & 3));
            }
        }
        if (packed && cnt == 4) { uint32_t* q = (uint32_t*)(out + p0 * 3); q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; }
        else for (int k = 0; k < cnt * 3; ++k) out[p0 * 3 + k] = (uint8_t)((o[k >> 2] >> (8 * (k & 3))) & 255u);
    }
}

// ================================================================= 16-bit apply (SPEC §6.20)
// The table of rule 9 at a 16-bit position: a value v stands for the grey level v / 257, the axis weights are (65535 - f, f), the eight corner weights integers below
// 2^48 — exact as doubles however they are formed, so the (db, dg) products are hoisted. 6 B in and 6 B out per pixel, four pixels (three 8-byte words) per thread.
#define LUT16_W3 281462092005375.0          // 65535^3: the sum of a pixel's eight integer weights
__device__ __forceinline__ void lut_axis16(int v, int N, int& i, int& f) {
    const int t = v * (N - 1);              // at most 65535 * 64
    i = min(t / 65535, N - 2);
    f = t - 65535 * i;
}
// pixels p0 .. p0 + 3 of a tightly packed 6-byte image as three 8-byte words (base 8-byte aligned, p0 a multiple of 4), else element by element; cnt <= 4 pixels are valid
__device__ __forceinline__ void lut_load4x16(const uint16_t* img, long p0, int cnt, bool packed, u64 w[3]) {
    if (packed && cnt == 4) {
        const u64* q = (const u64*)(img + p0 * 3);
        w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
    } else {
        w[0] = w[1] = w[2] = 0ull;
        for (int k = 0; k < cnt * 3; ++k) w[k >> 2] |= (u64)img[p0 * 3 + k] << (16 * (k & 3));
    }
}
__device__ __forceinline__ int lut_half(const u64 w[3], int k) { return (int)((w[k >> 2] >> (16 * (k & 3))) & 65535ull); }

template <bool IN_LDS>
__global__ __launch_bounds__(256) void k_lut_apply16(const float* __restrict__ lut, int N, const uint16_t* in, long npix, int packed, uint16_t* out) {   // out may be in
    __shared__ float sl[IN_LDS ? LUT_LDS_FLOATS : 1];
    const float* tab = lut;
    if (IN_LDS) {
        for (int i = threadIdx.x; i < N * N * N * 3; i += 256) sl[i] = lut[i];
        __syncthreads();
        tab = sl;
    }
    const long groups = (npix + 3) / 4;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const long p0 = g * 4;
        const int cnt = (int)min(4L, npix - p0);
        u64 w[3], o[3] = {0ull, 0ull, 0ull};
        lut_load4x16(in, p0, cnt, packed != 0, w);
        for (int j = 0; j < cnt; ++j) {
            int ib, fb, ig, fg, ir, fr;
            lut_axis16(lut_half(w, 3 * j), N, ib, fb); lut_axis16(lut_half(w, 3 * j + 1), N, ig, fg); lut_axis16(lut_half(w, 3 * j + 2), N, ir, fr);
            const double wr[2] = {(double)(65535 - fr), (double)fr};
            double acc[3] = {0.0, 0.0, 0.0};
            for (int pair = 0; pair < 4; ++pair) {
                const int db = pair >> 1, dg = pair & 1;
                const double wbg = (double)(db ? fb : 65535 - fb) * (double)(dg ? fg : 65535 - fg);      // below 2^32: exact
                const float* t = tab + (size_t)(((ib + db) * N + ig + dg) * N + ir) * 3;
                for (int dr = 0; dr < 2; ++dr) {
                    const double wt = wbg * wr[dr];                                                       // below 2^48: exact
                    for (int c = 0; c < 3; ++c) acc[c] += wt * (double)t[3 * dr + c];
                }
            }
            for (int c = 0; c < 3; ++c) {
                double v = acc[c] / LUT16_W3;
                v = v * 257.0;
                v = v > 0.0 ? v : 0.0; v = v < 65535.0 ? v : 65535.0;                   // A1's cast: clamp, then round to nearest even
                const int k = 3 * j + c;
                o[k >> 2] |= (u64)(unsigned)(int)rint(v) << (16 * (k & 3));
            }
        }
        if (packed && cnt == 4) { u64* q = (u64*)(out + p0 * 3); q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; }
        else for (int k = 0; k < cnt * 3; ++k) out[p0 * 3 + k] = (uint16_t)((o[k >> 2] >> (16 * (k & 3))) & 65535ull);
    }
}

// ================================================================= launchers
bool nct_lut_size_ok(int N) { return N == 3 || N == 5 || N == 9 || N == 17 || N == 33 || N == 65; }

int nctk_lut_accum_zero(nct_ctx* ctx, hipStream_t s, int N, uint64_t* W, int64_t* R, uint64_t* kept) {
    const size_t n3 = (size_t)N * N * N;
    NCT_HIP(hipMemsetAsync(W, 0, n3 * sizeof(uint64_t), s));
    NCT_HIP(hipMemsetAsync(R, 0, n3 * 3 * sizeof(int64_t), s));
    if (kept) NCT_HIP(hipMemsetAsync(kept, 0, sizeof(uint64_t), s));
    return NCT_OK;
}

int nctk_lut_splat(nct_ctx* ctx, hipStream_t s, const uint8_t* src, const uint8_t* res, long npix, int N, uint64_t* W, int64_t* R, bool accumulate) {
    // the arena clears nothing: the accumulators are zeroed on the stream in front of the splat (accumulate: they hold the sums of earlier splats, SPEC §6.20)
    if (!accumulate) NCT_TRY(nctk_lut_accum_zero(ctx, s, N, W, R, nullptr));
    long chunk = (npix + 1023) / 1024;                       // at most 1024 workgroups, each a contiguous run of at least 1024 pixels
    chunk = chunk < 1024 ? 1024 : (chunk + 3) / 4 * 4;
    const int grid = (int)((npix + chunk - 1) / chunk);
    const int packed = (((uintptr_t)src | (uintptr_t)res) & 3) == 0;
    k_lut_splat<<<grid, 256, 0, s>>>(src, res, npix, chunk, N, packed, (u64*)W, (u64*)R);
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}

int nctk_lut_splat_masked(nct_ctx* ctx, hipStream_t s, const uint8_t* src, const uint8_t* res, const uint8_t* mask, long npix, int N, uint64_t* W, int64_t* R, uint64_t* kept,
                          bool accumulate) {
    if (!accumulate) NCT_TRY(nctk_lut_accum_zero(ctx, s, N, W, R, kept));
    long chunk = (npix + 1023) / 1024;                       // the grid of nctk_lut_splat
    chunk = chunk < 1024 ? 1024 : (chunk + 3) / 4 * 4;
    const int grid = (int)((npix + chunk - 1) / chunk);
    const int packed = (((uintptr_t)src | (uintptr_t)res) & 3) == 0;
    k_lut_splat_masked<<<grid, 256, 0, s>>>(src, res, mask, npix, chunk, N, packed, (u64*)W, (u64*)R, (u64*)kept);
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}

int nctk_lut_solve(nct_ctx* ctx, hipStream_t s, const uint64_t* W, const int64_t* R, int N, double lambda, double* D) {
    lut_hier h; h.nlev = 0;
    DevBuf<double> A[LUT_MAXLEV], q[LUT_MAXLEV], x[LUT_MAXLEV], t[LUT_MAXLEV], b[LUT_MAXLEV], r[LUT_MAXLEV], ldl(ctx, 27 * 27 + 27);
    if (!ldl.ok()) return NCT_ERR_HIP;
    h.ldl = ldl;
    for (int n = N;; n = (n + 1) / 2) {
        const int k = h.nlev++;
        const size_t n3 = (size_t)n * n * n;
        if (!A[k].alloc(ctx, n3 * 27) || !q[k].alloc(ctx, n3) || !t[k].alloc(ctx, n3 * 3) || !b[k].alloc(ctx, n3 * 3) || !r[k].alloc(ctx, n3 * 3)) return NCT_ERR_HIP;
        if (k > 0 && !x[k].alloc(ctx, n3 * 3)) return NCT_ERR_HIP;
        h.lv[k] = lut_level{n, A[k], q[k], k > 0 ? (double*)x[k] : D, t[k], b[k], r[k]};
        if (n == 3) break;
    }
    int k0 = 0;
    while (h.lv[k0].n > LUT_TAIL_N) ++k0;
    auto grid = [](const lut_level& l, int per_node) { return cdiv(l.n * l.n * l.n * per_node, 256); };
    k_lut_fine<<<grid(h.lv[0], 1), 256, 0, s>>>((const u64*)W, (const long long*)R, lambda, h.lv[0]);
    NCT_LAUNCH_CHECK();
    for (int k = 0; k < k0; ++k) {
        k_lut_divisor<<<grid(h.lv[k], 1), 256, 0, s>>>(h.lv[k]);
        k_lut_galerkin<<<grid(h.lv[k + 1], 27), 256, 0, s>>>(h.lv[k], h.lv[k + 1]);
    }
    k_lut_tail_setup<<<1, 1024, 0, s>>>(h, k0);
    NCT_LAUNCH_CHECK();
    if (h.nlev == 1 || k0 == 0) {                               // the whole hierarchy in one workgroup: every cycle in one launch (N = 3: the direct solve alone)
        k_lut_tail_cycle<<<1, 1024, 0, s>>>(h, 0, h.nlev == 1 ? 1 : NCT_LUT_CYCLES);
        NCT_LAUNCH_CHECK();
        return NCT_OK;
    }
    for (int it = 0; it < NCT_LUT_CYCLES; ++it) {
        for (int k = 0; k < k0; ++k) {
            const lut_level& l = h.lv[k];
            k_lut_smooth<<<grid(l, 3), 256, 0, s>>>(l, l.x, l.t);
            k_lut_smooth<<<grid(l, 3), 256, 0, s>>>(l, l.t, l.x);
            k_lut_residual<<<grid(l, 3), 256, 0, s>>>(l);
            k_lut_restrict<<<grid(h.lv[k + 1], 3), 256, 0, s>>>(l, h.lv[k + 1]);
        }
        k_lut_tail_cycle<<<1, 1024, 0, s>>>(h, k0, 1);
        for (int k = k0 - 1; k >= 0; --k) {
            const lut_level& l = h.lv[k];
            k_lut_prolong_add<<<grid(l, 3), 256, 0, s>>>(l, h.lv[k + 1]);
            k_lut_smooth<<<grid(l, 3), 256, 0, s>>>(l, l.x, l.t);
            k_lut_smooth<<<grid(l, 3), 256, 0, s>>>(l, l.t, l.x);
        }
        NCT_LAUNCH_CHECK();
    }
    return NCT_OK;
}

int nctk_lut_table(nct_ctx* ctx, hipStream_t s, const double* D, int N, float* lut) {
    k_lut_table<<<cdiv(N * N * N * 3, 256), 256, 0, s>>>(D, N, lut);
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}

int nctk_lut_apply(nct_ctx* ctx, hipStream_t s, const float* lut, int N, const uint8_t* in, long npix, uint8_t* out) {
    const long groups = (npix + 3) / 4;
    const int packed = (((uintptr_t)in | (uintptr_t)out) & 3) == 0;
    long grid = (groups + 255) / 256;
    if (N <= 17) {
        if (grid > 1024) grid = 1024;                           // every workgroup copies the table once: 1024 copies of 59 KB at most
        k_lut_apply<true><<<(int)grid, 256, 0, s>>>(lut, N, in, npix, packed, out);
    } else {
        if (grid > 8192) grid = 8192;
        k_lut_apply<false><<<(int)grid, 256, 0, s>>>(lut, N, in, npix, packed, out);
    }
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}

int nctk_lut_apply16(nct_ctx* ctx, hipStream_t s, const float* lut, int N, const uint16_t* in, long npix, uint16_t* out) {
    const long groups = (npix + 3) / 4;
    const int packed = (((uintptr_t)in | (uintptr_t)out) & 7) == 0;
    long grid = (groups + 255) / 256;                               // the grids of nctk_lut_apply
    if (N <= 17) {
        if (grid > 1024) grid = 1024;
        k_lut_apply16<true><<<(int)grid, 256, 0, s>>>(lut, N, in, npix, packed, out);
    } else {
        if (grid > 8192) grid = 8192;
        k_lut_apply16<false><<<(int)grid, 256, 0, s>>>(lut, N, in, npix, packed, out);
    }
    NCT_LAUNCH_CHECK();
    return NCT_OK;
}
