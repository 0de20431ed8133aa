// k_region_snap.hip — snapping a region matte to the edges of its frame (SPEC §6.15). k_region_snap is a joint filter over the matte (H x W bytes) with the frame's 8-bit
// Lab image as the guide: per pixel p the taps q of the (2r + 1)^2 window that lie inside the image weigh w(q) = max(0, 3 sigma^2 - |Lab(p) - Lab(q)|^2), and the output
// is the weighted mean of the matte rounded half up, or with `binary` that mean cut at 128. Integers only: the result does not depend on the order of the taps.
//
// MI355X design: the shape of the finish passes and of k_seq_matte_warp. One workgroup = one 32 x 8 tile of target pixels. The tile and its halo, (32 + 2r) x (8 + 2r)
// pixels, are staged in LDS once, one packed 32-bit word per pixel (L, a, b, matte from the low byte up): 4 B in and 1 B out per pixel beside the halo, which the
// neighbouring tiles' loads leave in L2. Positions outside the image hold 0 and are never read: a pixel's tap loops run over the part of its window inside the
// image, so a skipped tap costs nothing and no flag is needed. Then (2r + 1)^2 ds_read_b32 per pixel, each followed by three byte differences, the weight and two
// accumulations.
// LDS layout: a row stride of 32 + 2r + 1 words, odd on purpose. ds_read_b32 banks are (address / 4) mod 32 and conflicts count within each 32-lane half. With one
// pixel per thread a half-wave is one tile row: 32 consecutive words, conflict-free at any stride. With four pixels per thread a half-wave is 4 rows x 8 threads whose
// words are 4 apart in a row: the banks are (ty * stride + 4 tx + c) mod 32, distinct exactly where ty * stride mod 4 takes four values, i.e. for an odd stride.
// At r = 8 the tile is 49 x 24 words = 4704 B.
// Ranges: d2 <= 3 * 255^2 = 195075 and w <= 3 sigma^2 <= 195075 < 2^18 fit 32 bits; B <= 289 w < 2^26 is accumulated in 32 bits; A <= 255 B < 2^34 needs 64
// (summing a window row in 32 bits first and adding it to A once per row was measured 15 % slower at every radius: the per-tap 64-bit add is kept).
// The division: n = 2A + B < 2^35, d = 2B < 2^27 and the quotient is below 256, so the correctly rounded float quotient of the two rounded operands (relative error
// below 2^-22, absolute below 2^-14) is within one of the floor; the exact 64-bit remainder corrects it. With `binary` no division is needed: v >= 128 <=> n >= 128 d.
// r is a runtime argument: the tap loops are bounded per pixel anyway.
#include "nct_internal.h"
#include "nct_device.h"

#define RS_TX 32
#define RS_TY 8
#define RS_RMAX 8
#define RS_LW_MAX (RS_TX + 2 * RS_RMAX + 1)
#define RS_LH_MAX (RS_TY + 2 * RS_RMAX)

// SPEC §6.15 rule 1 for one pixel whose window is staged around LDS word `c` (its own): rows dy0 … dy1, columns dx0 … dx1 of the window lie inside the image
__device__ __forceinline__ uint8_t rs_pixel(const uint32_t* c, int lw, int dy0, int dy1, int dx0, int dx1, int s3, int binary) {
    const uint32_t p = *c;
    const int pl = p & 0xffu, pa = (p >> 8) & 0xffu, pb = (p >> 16) & 0xffu;
    unsigned long long A = 0; uint32_t B = 0;
    for (int dy = dy0; dy <= dy1; ++dy) {
        const uint32_t* row = c + dy * lw;
        for (int dx = dx0; dx <= dx1; ++dx) {
            const uint32_t q = row[dx];
            const int dl = (int)(q & 0xffu) - pl, da = (int)((q >> 8) & 0xffu) - pa, db = (int)((q >> 16) & 0xffu) - pb;
            const int w = max(0, s3 - (dl * dl + da * da + db * db));
            A += (unsigned long long)((uint32_t)w * (q >> 24));
            B += (uint32_t)w;
        }
    }
    const unsigned long long n = 2 * A + B, d = 2ull * B;      // B >= 3 sigma^2 > 0: the centre tap
    if (binary) return n >= 128 * d ? 255 : 0;
    long long v = (long long)((float)n / (float)d);
    long long rem = (long long)n - v * (long long)d;
    while (rem < 0) { rem += (long long)d; --v; }
    while (rem >= (long long)d) { rem -= (long long)d; ++v; }
    return (uint8_t)v;
}

// V pixels per thread along x (1 or 4); the block is (RS_TX / V) x RS_TY threads
template <int V>
__global__ __launch_bounds__(RS_TX * RS_TY / V) void k_region_snap(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ lab, int H, int W, int r, int s3, int binary,
                                                                   uint8_t* __restrict__ out) {
    __shared__ uint32_t tile[RS_LH_MAX * RS_LW_MAX];
    const int x0 = blockIdx.x * RS_TX, y0 = blockIdx.y * RS_TY;
    const int tw = RS_TX + 2 * r, th = RS_TY + 2 * r, lw = tw + 1;             // r <= RS_RMAX: th * lw fits the tile
    const int tid = threadIdx.y * (RS_TX / V) + threadIdx.x;
    for (int e = tid; e < tw * th; e += RS_TX * RS_TY / V) {
        const int py = e / tw, px = e - py * tw;
        const int gy = y0 - r + py, gx = x0 - r + px;
        uint32_t word = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t g = (size_t)gy * W + gx;
            word = (uint32_t)lab[3 * g] | (uint32_t)lab[3 * g + 1] << 8 | (uint32_t)lab[3 * g + 2] << 16 | (uint32_t)mask[g] << 24;
        }
        tile[py * lw + px] = word;
    }
    __syncthreads();
    const int xb = x0 + threadIdx.x * V, y = y0 + threadIdx.y;
    if (xb >= W || y >= H) return;
    // the window's rows inside the image; y - y0 + r + dy stays in [0, th)
    const int dy0 = -min(r, y), dy1 = min(r, H - 1 - y);
    const uint32_t* crow = tile + (threadIdx.y + r) * lw + threadIdx.x * V + r;
    uint32_t packed = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int x = xb + v;
        if (x >= W) break;
        const uint8_t b = rs_pixel(crow + v, lw, dy0, dy1, -min(r, x), min(r, W - 1 - x), s3, binary);
        if (V == 1) out[(size_t)y * W + x] = b;
        else packed |= (uint32_t)b << (8 * v);
    }
    // W % 4 == 0 and xb % 4 == 0: the four pixels are inside the row together, and the dword is aligned where `out` is
    if (V == 4) *(uint32_t*)(out + (size_t)y * W + xb) = packed;
}

void nct_region_snap_params_default(nct_region_snap_params* p) {
    if (!p) return;
    p->radius = 3; p->sigma = 10; p->binary = 1;
}

int nct_region_snap_params_check(nct_ctx* ctx, const char* who, const nct_region_snap_params* p) {
    if (!p) return 0;
    NCT_REQUIRE(p->radius >= 1 && p->radius <= RS_RMAX, "%s: radius must be in [1, %d] (got %d)", who, RS_RMAX, p->radius);
    NCT_REQUIRE(p->sigma >= 1 && p->sigma <= 255, "%s: sigma must be in [1, 255] (got %d)", who, p->sigma);
    NCT_REQUIRE(p->binary == 0 || p->binary == 1, "%s: binary must be 0 or 1 (got %d)", who, p->binary);
    return 0;
}

int nct_region_snap_check(nct_ctx* ctx, const char* who, const void* mask, const void* lab, int H, int W, const nct_region_snap_params* p, const void* mask_out) {
    NCT_REQUIRE(mask, "%s: null mask", who);
    NCT_REQUIRE(lab, "%s: null lab", who);
    NCT_REQUIRE(mask_out, "%s: null mask_out", who);
    NCT_REQUIRE(H >= 1 && W >= 1 && H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS,
                "%s: size H x W = %dx%d outside [1, %d] per side or above %lld pixels", who, H, W, NCT_FINISH_MAX_SIDE, (long long)NCT_FINISH_MAX_PIXELS);
    return nct_region_snap_params_check(ctx, who, p);
}

int nctk_region_snap(nct_ctx* ctx, hipStream_t s, const uint8_t* mask, const uint8_t* lab, int H, int W, const nct_region_snap_params* params, uint8_t* mask_out) {
    NCT_TRY(nct_region_snap_check(ctx, "region_snap", mask, lab, H, W, params, mask_out));
    // the kernel reads mask and lab at other pixels than the one it writes: any overlap with the output is refused
    const char *o = (const char*)mask_out, *m = (const char*)mask, *l = (const char*)lab;
    const size_t bytes = (size_t)H * W;
    NCT_REQUIRE(o + bytes <= m || m + bytes <= o, "region_snap: mask_out must not alias mask");
    NCT_REQUIRE(o + bytes <= l || l + 3 * bytes <= o, "region_snap: mask_out must not alias lab");
    nct_region_snap_params p;
    if (params) p = *params; else nct_region_snap_params_default(&p);
    const int s3 = 3 * p.sigma * p.sigma;
    const dim3 grid(cdiv(W, RS_TX), cdiv(H, RS_TY));
    if (W % 4 == 0 && ((uintptr_t)mask_out & 3) == 0)
        hipLaunchKernelGGL(k_region_snap<4>, grid, dim3(RS_TX / 4, RS_TY), 0, s, mask, lab, H, W, p.radius, s3, p.binary, mask_out);
    else
        hipLaunchKernelGGL(k_region_snap<1>, grid, dim3(RS_TX, RS_TY), 0, s, mask, lab, H, W, p.radius, s3, p.binary, mask_out);
    NCT_LAUNCH_CHECK();
    return 0;
}
