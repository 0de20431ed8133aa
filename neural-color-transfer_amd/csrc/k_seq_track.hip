// k_seq_track.hip — carrying a sequence's region matte along the motion field (SPEC §6.14). k_seq_matte_warp pulls the previous frame's matte (H x W bytes) through a
// level's backward field (h x w int16 pairs (my, mx), h <= H, w <= W): per target pixel the field is interpolated at the pixel's centre-aligned position on the level
// grid — nct_resize's index rule as an exact fraction — scaled to target pixels and rounded half up, all in integers; then one byte is copied from the clamped
// position. A byte is never interpolated: a binary matte stays binary, and nothing blurs over a shot.
//
// MI355X design: the shape of the finish passes. One workgroup = one 32 x 8 tile of target pixels. The field taps the tile interpolates — at most 34 x 10 vectors at
// a ratio >= 1, bounded by the first pixel's s and the last pixel's s1 — are staged in LDS once, one 32-bit word per vector (1360 B). Then per pixel four LDS words,
// one gathered byte and one stored byte: 1 B in, 1 B out per pixel beside the (smaller) field. Where W % 4 == 0 and the output is dword aligned a thread takes four
// consecutive pixels and stores one dword (the workgroup is then one wave of 8 x 8 threads); else one thread per pixel and byte stores.
// The two divisions of the rule have divisors that are uniform over the launch (2 h Dy Dx and 2 w Dy Dx, below 2^41) and numerators below 2^60: the quotient is
// estimated with the divisor's double reciprocal (the estimate is within one of the floor: the relative error is 2^-51, the quotient below 2^31) and corrected with
// the exact 64-bit remainder, so the result is the floor division's and no 64-bit integer division is emitted.
#include "nct_internal.h"
#include "nct_device.h"

#define MW_TX 32
#define MW_TY 8
#define MW_LW (MW_TX + 2)
#define MW_LH (MW_TY + 2)

// SPEC §6.14 rule 1 for one axis: target coordinate x of W on a grid of w -> the two taps and the numerator t of the fraction t / (2 W)
struct MwTap { int s, s1, t; };
__host__ __device__ __forceinline__ MwTap mw_tap(int x, int w, int W) {
    const int D = 2 * W, num = (2 * x + 1) * w - W;             // num > -D: its floor quotient is -1 where it is negative
    int s = num < 0 ? -1 : num / D;
    int t = num - s * D;
    if (s < 0) { s = 0; t = 0; }
    if (s >= w - 1) { s = w - 1; t = 0; }
    MwTap r; r.s = s; r.s1 = s + 1 < w - 1 ? s + 1 : w - 1; r.t = t;
    return r;
}

// floor(n / d) for d > 0, |n / d| < 2^31: the double estimate, then the exact remainder decides
__device__ __forceinline__ int mw_floor_div(long long n, long long d, double inv_d) {
    long long q = (long long)floor((double)n * inv_d);
    long long r = n - q * d;
    while (r < 0) { r += d; --q; }
    while (r >= d) { r -= d; ++q; }
    return (int)q;
}

// V pixels per thread along x (1 or 4); the block is (MW_TX / V) x MW_TY threads
template <int V>
__global__ __launch_bounds__(MW_TX * MW_TY / V) void k_seq_matte_warp(const uint8_t* __restrict__ prev, int H, int W, const uint32_t* __restrict__ field, int h, int w,
                                                                      double inv_dy, double inv_dx, uint8_t* __restrict__ out) {
    __shared__ uint32_t tile[MW_LH * MW_LW];
    const int x0 = blockIdx.x * MW_TX, y0 = blockIdx.y * MW_TY;
    const int x1 = min(x0 + MW_TX, W) - 1, y1 = min(y0 + MW_TY, H) - 1;
    // the staged region: from the first pixel's s to the last pixel's s1 (both monotonic in the coordinate), never wider than the tile's LDS
    const int sx_lo = mw_tap(x0, w, W).s, sy_lo = mw_tap(y0, h, H).s;
    const int tw = min(mw_tap(x1, w, W).s1 - sx_lo + 1, MW_LW), th = min(mw_tap(y1, h, H).s1 - sy_lo + 1, MW_LH);
    const int tid = threadIdx.y * (MW_TX / V) + threadIdx.x;
    for (int e = tid; e < tw * th; e += MW_TX * MW_TY / V) {
        const int py = e / tw, px = e - py * tw;
        tile[py * MW_LW + px] = field[(size_t)min(sy_lo + py, h - 1) * w + min(sx_lo + px, w - 1)];
    }
    __syncthreads();
    const int xb = x0 + threadIdx.x * V, y = y0 + threadIdx.y;
    if (xb >= W || y >= H) return;
    const long long Dy = 2LL * H, Dx = 2LL * W;
    const long long den_y = (long long)h * Dy * Dx, den_x = (long long)w * Dy * Dx;
    const MwTap cy = mw_tap(y, h, H);
    const int ly0 = min(cy.s - sy_lo, th - 1) * MW_LW, ly1 = min(cy.s1 - sy_lo, th - 1) * MW_LW;
    uint32_t packed = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int x = xb + v;
        if (x >= W) break;
        const MwTap cx = mw_tap(x, w, W);
        const int lx0 = min(cx.s - sx_lo, tw - 1), lx1 = min(cx.s1 - sx_lo, tw - 1);
        const uint32_t f00 = tile[ly0 + lx0], f01 = tile[ly0 + lx1], f10 = tile[ly1 + lx0], f11 = tile[ly1 + lx1];
        const long long w00 = (Dy - cy.t) * (Dx - cx.t), w01 = (Dy - cy.t) * cx.t, w10 = cy.t * (Dx - cx.t), w11 = (long long)cy.t * cx.t;
        // a vector's word: my in the low half, mx in the high half
        const long long Sy = w00 * (short)(f00 & 0xffffu) + w01 * (short)(f01 & 0xffffu) + w10 * (short)(f10 & 0xffffu) + w11 * (short)(f11 & 0xffffu);
        const long long Sx = w00 * (short)(f00 >> 16) + w01 * (short)(f01 >> 16) + w10 * (short)(f10 >> 16) + w11 * (short)(f11 >> 16);
        const int dy = mw_floor_div(2 * Sy * H + den_y, 2 * den_y, inv_dy), dx = mw_floor_div(2 * Sx * W + den_x, 2 * den_x, inv_dx);
        const uint8_t b = prev[(size_t)clampi(y + dy, 0, H - 1) * W + clampi(x + dx, 0, W - 1)];
        if (V == 1) out[(size_t)y * W + x] = b;
        else packed |= (uint32_t)b << (8 * v);
    }
    // W % 4 == 0 and xb % 4 == 0: the four pixels are inside the row together, and the dword is aligned where `out` is
    if (V == 4) *(uint32_t*)(out + (size_t)y * W + xb) = packed;
}

int nct_seq_matte_warp_check(nct_ctx* ctx, const char* who, const void* mask_prev, int H, int W, const void* field, int h, int w, const void* mask_out) {
    NCT_REQUIRE(mask_prev, "%s: null mask_prev", who);
    NCT_REQUIRE(field, "%s: null field", who);
    NCT_REQUIRE(mask_out, "%s: null mask_out", who);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "%s: field grid h x w = %dx%d outside [1, 4096] per side", who, h, w);
    NCT_REQUIRE(H >= 1 && W >= 1 && H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS,
                "%s: target H x W = %dx%d outside [1, %d] per side or above %lld pixels", who, H, W, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    NCT_REQUIRE(H >= h && W >= w, "%s: target H x W = %dx%d smaller than the field grid h x w = %dx%d", who, H, W, h, w);
    NCT_REQUIRE(((uintptr_t)field & 3) == 0, "%s: field must be aligned to its 4-byte vectors", who);
    return 0;
}

int nctk_seq_matte_warp(nct_ctx* ctx, hipStream_t s, const uint8_t* mask_prev, int H, int W, const int16_t* field, int h, int w, uint8_t* mask_out) {
    NCT_TRY(nct_seq_matte_warp_check(ctx, "seq_matte_warp", mask_prev, H, W, field, h, w, mask_out));
    // the kernel reads mask_prev at other pixels than the one it writes: any overlap of the two mattes is refused
    const size_t bytes = (size_t)H * W;
    NCT_REQUIRE((const char*)mask_out + bytes <= (const char*)mask_prev || (const char*)mask_prev + bytes <= (const char*)mask_out, "seq_matte_warp: mask_out must not alias mask_prev");
    const double inv_dy = 1.0 / (2.0 * h * (2.0 * H) * (2.0 * W)), inv_dx = 1.0 / (2.0 * w * (2.0 * H) * (2.0 * W));
    const dim3 grid(cdiv(W, MW_TX), cdiv(H, MW_TY));
    if (W % 4 == 0 && ((uintptr_t)mask_out & 3) == 0)
        hipLaunchKernelGGL(k_seq_matte_warp<4>, grid, dim3(MW_TX / 4, MW_TY), 0, s, mask_prev, H, W, (const uint32_t*)field, h, w, inv_dy, inv_dx, mask_out);
    else
        hipLaunchKernelGGL(k_seq_matte_warp<1>, grid, dim3(MW_TX, MW_TY), 0, s, mask_prev, H, W, (const uint32_t*)field, h, w, inv_dy, inv_dx, mask_out);
    NCT_LAUNCH_CHECK();
    return 0;
}
