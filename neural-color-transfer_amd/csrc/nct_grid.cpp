// nct_grid.cpp — C ABI of the local colour grids (SPEC §6.22): fit from a (source, result) pair, apply to 8-bit and 16-bit pixels, on host and on device pointers.
#include "nct_internal.h"
#include <cmath>

#define NCT_GRID_NSUM 22

static int grid_dims_check(nct_ctx* ctx, const char* what, int gy, int gx, int gz) {
    NCT_REQUIRE(gy >= 2 && gy <= 64 && gx >= 2 && gx <= 64, "%s: gy and gx must be in [2, 64] (got %d, %d)", what, gy, gx);
    NCT_REQUIRE(gz >= 2 && gz <= 32, "%s: gz must be in [2, 32] (got %d)", what, gz);
    return NCT_OK;
}
static int grid_image_check(nct_ctx* ctx, const char* what, int h, int w) {
    NCT_REQUIRE(h >= 1 && h <= NCT_GRID_MAX_SIDE && w >= 1 && w <= NCT_GRID_MAX_SIDE, "%s: h and w must be in [1, %d] (got %d, %d)", what, NCT_GRID_MAX_SIDE, h, w);
    NCT_REQUIRE((size_t)h * w <= (size_t)NCT_LUT_MAX_PIXELS, "%s: the number of pixels h * w must be at most 2^26 (got %zu)", what, (size_t)h * w);
    return NCT_OK;
}

int nct_grid_fit_check(nct_ctx* ctx, const char* what, const void* src, const void* res, int h, int w, const nct_grid_params* prm, const void* grid_out) {
    NCT_REQUIRE(src && res && prm && grid_out, "%s: null pointer", what);
    NCT_TRY(grid_image_check(ctx, what, h, w));
    NCT_TRY(grid_dims_check(ctx, what, prm->gy, prm->gx, prm->gz));
    NCT_REQUIRE(std::isfinite(prm->lambda) && prm->lambda >= 1.0 / 16.0 && prm->lambda <= 65536.0, "%s: lambda must be finite and in [1/16, 65536] (got %g)", what, prm->lambda);
    return NCT_OK;
}

int nct_grid_fit_enqueue(nct_ctx* ctx, const uint8_t* d_src, const uint8_t* d_res, int h, int w, const nct_grid_params* prm, double* d_grid, const nct_grid_stages* st) {
    const size_t n = (size_t)prm->gy * prm->gx * prm->gz * NCT_GRID_NSUM;
    // a stage the caller asks for is computed in the caller's array; the others in arena blocks that go back in stream order
    DevBuf<int64_t> sums, blurred;
    int64_t* S = st && st->sums ? st->sums : nullptr;
    int64_t* B = st && st->blurred ? st->blurred : nullptr;
    if (!S) { if (!sums.alloc(ctx, n)) return NCT_ERR_HIP; S = sums; }
    if (!B) { if (!blurred.alloc(ctx, n)) return NCT_ERR_HIP; B = blurred; }
    NCT_TRY(nctk_grid_splat(ctx, ctx->stream, d_src, d_res, h, w, prm->gy, prm->gx, prm->gz, S));
    return nctk_grid_solve(ctx, ctx->stream, S, prm->gy, prm->gx, prm->gz, prm->lambda, B, d_grid);
}

static int grid_apply_check(nct_ctx* ctx, const char* what, const void* grid, int gy, int gx, int gz, const void* bgr, int h, int w, const void* out) {
    NCT_REQUIRE(grid && bgr && out, "%s: null pointer", what);
    NCT_TRY(grid_dims_check(ctx, what, gy, gx, gz));
    return grid_image_check(ctx, what, h, w);
}

// the two host applies: the same call on pixels of another depth
template <typename T, typename F>
static int grid_apply_host(nct_ctx* ctx, const char* what, const double* grid, int gy, int gx, int gz, const T* bgr, int h, int w, T* out, F launch) {
    NCT_TRY(grid_apply_check(ctx, what, grid, gy, gx, gz, bgr, h, w, out));
    const size_t n = (size_t)gy * gx * gz * 12, npix = (size_t)h * w;
    for (size_t i = 0; i < n; ++i) NCT_REQUIRE(std::isfinite(grid[i]), "%s: the grid has a non-finite entry (node %zu, coefficient %zu)", what, i / 12, i % 12);
    HostCall hc(ctx);
    const double* dg = hc.in(grid, n);
    const T* di = hc.in(bgr, npix * 3);
    T* dout = hc.out(out, npix * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(launch(ctx, ctx->stream, dg, gy, gx, gz, di, h, w, dout));
    return hc.finish();
}

extern "C" {

void nct_grid_params_default(nct_grid_params* p) {
    if (!p) return;
    p->gy = p->gx = p->gz = 16; p->lambda = 16.0;
}

int nct_grid_fit(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, int h, int w, const nct_grid_params* prm, double* grid_out, nct_grid_stages* stages) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_grid_fit_check(ctx, "grid_fit", src_bgr, res_bgr, h, w, prm, grid_out));
    const size_t nodes = (size_t)prm->gy * prm->gx * prm->gz, npix = (size_t)h * w;
    HostCall hc(ctx);
    const uint8_t *ds = hc.in(src_bgr, npix * 3), *dr = hc.in(res_bgr, npix * 3);
    double* dg = hc.out(grid_out, nodes * 12);
    // the two stages are computed in blocks of this call and come down where they are asked for
    int64_t* s = hc.scratch<int64_t>(nodes * NCT_GRID_NSUM); int64_t* b = hc.scratch<int64_t>(nodes * NCT_GRID_NSUM);
    if (stages) { hc.get(stages->sums, s, nodes * NCT_GRID_NSUM); hc.get(stages->blurred, b, nodes * NCT_GRID_NSUM); }
    NCT_TRY(hc.ready());
    const nct_grid_stages dst{s, b};
    NCT_TRY(nct_grid_fit_enqueue(ctx, ds, dr, h, w, prm, dg, &dst));
    return hc.finish();
}

int nct_grid_fit_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, int h, int w, const nct_grid_params* prm, double* d_grid_out, nct_grid_stages* d_stages) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_grid_fit_check(ctx, "grid_fit_dev", d_src_bgr, d_res_bgr, h, w, prm, d_grid_out));
    return nct_grid_fit_enqueue(ctx, d_src_bgr, d_res_bgr, h, w, prm, d_grid_out, d_stages);
}

int nct_grid_apply(nct_ctx* ctx, const double* grid, int gy, int gx, int gz, const uint8_t* bgr, int h, int w, uint8_t* out_bgr) {
    NCT_CTX_ENTER();
    return grid_apply_host(ctx, "grid_apply", grid, gy, gx, gz, bgr, h, w, out_bgr, nctk_grid_apply);
}

int nct_grid_apply_dev(nct_ctx* ctx, const double* d_grid, int gy, int gx, int gz, const uint8_t* d_bgr, int h, int w, uint8_t* d_out_bgr) {
    NCT_CTX_ENTER();
    NCT_TRY(grid_apply_check(ctx, "grid_apply_dev", d_grid, gy, gx, gz, d_bgr, h, w, d_out_bgr));
    return nctk_grid_apply(ctx, ctx->stream, d_grid, gy, gx, gz, d_bgr, h, w, d_out_bgr);
}

int nct_grid_apply_u16(nct_ctx* ctx, const double* grid, int gy, int gx, int gz, const uint16_t* bgr16, int h, int w, uint16_t* out_bgr16) {
    NCT_CTX_ENTER();
    return grid_apply_host(ctx, "grid_apply_u16", grid, gy, gx, gz, bgr16, h, w, out_bgr16, nctk_grid_apply16);
}

int nct_grid_apply_u16_dev(nct_ctx* ctx, const double* d_grid, int gy, int gx, int gz, const uint16_t* d_bgr16, int h, int w, uint16_t* d_out_bgr16) {
    NCT_CTX_ENTER();
    NCT_TRY(grid_apply_check(ctx, "grid_apply_u16_dev", d_grid, gy, gx, gz, d_bgr16, h, w, d_out_bgr16));
    return nctk_grid_apply16(ctx, ctx->stream, d_grid, gy, gx, gz, d_bgr16, h, w, d_out_bgr16);
}

}  // extern "C"
