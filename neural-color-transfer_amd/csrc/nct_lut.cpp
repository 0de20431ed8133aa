// nct_lut.cpp — C ABI of the 3D colour look-up tables (SPEC §6.6): fit from a (source, result) pair, apply, on host and on device pointers.
#include "nct_internal.h"
#include <cmath>

int nct_lut_fit_check(nct_ctx* ctx, const char* what, const void* src, const void* res, size_t npix, const nct_lut_params* prm, const void* lut_out) {
    NCT_REQUIRE(src && res && prm && lut_out, "%s: null pointer", what);
    NCT_REQUIRE(nct_lut_size_ok(prm->size), "%s: the lattice size must be one of 3, 5, 9, 17, 33, 65 (got %d)", what, prm->size);
    NCT_REQUIRE(std::isfinite(prm->lambda) && prm->lambda > 0.0, "%s: lambda must be finite and greater than 0 (got %g)", what, prm->lambda);
    NCT_REQUIRE(npix >= 1 && npix <= (size_t)NCT_LUT_MAX_PIXELS, "%s: the number of pixels must be in [1, 2^26] (got %zu)", what, npix);
    return NCT_OK;
}

// d_mask null: the fit of every pixel. Non-null (SPEC §6.11 rule 7): the masked splat, and a wait for it — a fit that kept no pixel is refused before the solve
static int lut_fit_run(nct_ctx* ctx, const char* what, const uint8_t* d_src, const uint8_t* d_res, const uint8_t* d_mask, size_t npix, const nct_lut_params* prm, float* d_lut,
                       const nct_lut_stages* st) {
    const int N = prm->size;
    const size_t n3 = (size_t)N * N * N;
    const hipStream_t s = ctx->stream;
    // a stage the caller asks for is computed in the caller's array; the others in arena blocks that go back in stream order
    DevBuf<uint64_t> w; DevBuf<int64_t> r; DevBuf<double> d;
    uint64_t* W = st && st->weight ? st->weight : nullptr;
    int64_t* R = st && st->resid ? st->resid : nullptr;
    double* D = st && st->disp ? st->disp : nullptr;
    if (!W) { if (!w.alloc(ctx, n3)) return NCT_ERR_HIP; W = w; }
    if (!R) { if (!r.alloc(ctx, n3 * 3)) return NCT_ERR_HIP; R = r; }
    if (!D) { if (!d.alloc(ctx, n3 * 3)) return NCT_ERR_HIP; D = d; }
    if (d_mask) {
        DevBuf<uint64_t> kept;
        if (!kept.alloc(ctx, 1)) return NCT_ERR_HIP;
        NCT_TRY(nctk_lut_splat_masked(ctx, s, d_src, d_res, d_mask, (long)npix, N, W, R, kept));
        uint64_t nkept = 0;
        NCT_D2H(&nkept, kept, sizeof nkept);
        NCT_SYNC();
        NCT_REQUIRE(nkept > 0, "%s: the mask keeps no pixel (none of the %zu has mask >= 128)", what, npix);
    } else NCT_TRY(nctk_lut_splat(ctx, s, d_src, d_res, (long)npix, N, W, R));
    NCT_TRY(nctk_lut_solve(ctx, s, W, R, N, prm->lambda, D));
    return nctk_lut_table(ctx, s, D, N, d_lut);
}
int nct_lut_fit_enqueue(nct_ctx* ctx, const uint8_t* d_src, const uint8_t* d_res, size_t npix, const nct_lut_params* prm, float* d_lut, const nct_lut_stages* st) {
    return lut_fit_run(ctx, "lut_fit", d_src, d_res, nullptr, npix, prm, d_lut, st);
}
int nct_lut_fit_enqueue_masked(nct_ctx* ctx, const char* what, const uint8_t* d_src, const uint8_t* d_res, const uint8_t* d_mask, size_t npix, const nct_lut_params* prm, float* d_lut,
                               const nct_lut_stages* st) {
    return lut_fit_run(ctx, what, d_src, d_res, d_mask, npix, prm, d_lut, st);
}

static int lut_apply_check(nct_ctx* ctx, const char* what, const void* lut, int size, const void* bgr, size_t npix, const void* out) {
    NCT_REQUIRE(lut && bgr && out, "%s: null pointer", what);
    NCT_REQUIRE(nct_lut_size_ok(size), "%s: the lattice size must be one of 3, 5, 9, 17, 33, 65 (got %d)", what, size);
    NCT_REQUIRE(npix >= 1 && npix <= (size_t)NCT_LUT_MAX_PIXELS, "%s: the number of pixels must be in [1, 2^26] (got %zu)", what, npix);
    return NCT_OK;
}

extern "C" {

void nct_lut_params_default(nct_lut_params* p) {
    if (!p) return;
    p->size = 33; p->lambda = 0.1;
}

int nct_lut_fit(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, size_t npix, const nct_lut_params* prm, float* lut_out, nct_lut_stages* stages) {
    return nct_lut_fit_masked(ctx, src_bgr, res_bgr, nullptr, npix, prm, lut_out, stages);
}

int nct_lut_fit_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, size_t npix, const nct_lut_params* prm, float* d_lut_out, nct_lut_stages* d_stages) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_lut_fit_check(ctx, "lut_fit_dev", d_src_bgr, d_res_bgr, npix, prm, d_lut_out));
    return nct_lut_fit_enqueue(ctx, d_src_bgr, d_res_bgr, npix, prm, d_lut_out, d_stages);
}

// SPEC §6.11 rule 7: the fit over the pixels with mask >= 128; mask NULL: nct_lut_fit
int nct_lut_fit_masked(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, const uint8_t* mask, size_t npix, const nct_lut_params* prm, float* lut_out, nct_lut_stages* stages) {
    NCT_CTX_ENTER();
    const char* what = mask ? "lut_fit_masked" : "lut_fit";
    NCT_TRY(nct_lut_fit_check(ctx, what, src_bgr, res_bgr, npix, prm, lut_out));
    const size_t n3 = (size_t)prm->size * prm->size * prm->size;
    HostCall hc(ctx);
    const uint8_t *ds = hc.in(src_bgr, npix * 3), *dr = hc.in(res_bgr, npix * 3), *dm = hc.in(mask, npix);
    float* dl = hc.out(lut_out, n3 * 3);
    // the three stages are computed in blocks of this call and come down where they are asked for
    uint64_t* w = hc.scratch<uint64_t>(n3); int64_t* r = hc.scratch<int64_t>(n3 * 3); double* d = hc.scratch<double>(n3 * 3);
    if (stages) { hc.get(stages->weight, w, n3); hc.get(stages->resid, r, n3 * 3); hc.get(stages->disp, d, n3 * 3); }
    NCT_TRY(hc.ready());
    const nct_lut_stages dst{w, r, d};
    NCT_TRY(lut_fit_run(ctx, what, ds, dr, dm, npix, prm, dl, &dst));
    return hc.finish();
}

int nct_lut_fit_masked_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, const uint8_t* d_mask, size_t npix, const nct_lut_params* prm, float* d_lut_out,
                           nct_lut_stages* d_stages) {
    if (!d_mask) return nct_lut_fit_dev(ctx, d_src_bgr, d_res_bgr, npix, prm, d_lut_out, d_stages);
    NCT_CTX_ENTER();
    NCT_TRY(nct_lut_fit_check(ctx, "lut_fit_masked_dev", d_src_bgr, d_res_bgr, npix, prm, d_lut_out));
    return nct_lut_fit_enqueue_masked(ctx, "lut_fit_masked_dev", d_src_bgr, d_res_bgr, d_mask, npix, prm, d_lut_out, d_stages);
}

int nct_lut_apply(nct_ctx* ctx, const float* lut, int size, const uint8_t* bgr, size_t npix, uint8_t* out_bgr) {
    NCT_CTX_ENTER();
    NCT_TRY(lut_apply_check(ctx, "lut_apply", lut, size, bgr, npix, out_bgr));
    const size_t n = (size_t)size * size * size * 3;
    for (size_t i = 0; i < n; ++i) NCT_REQUIRE(std::isfinite(lut[i]), "lut_apply: the table has a non-finite entry (node %zu, channel %zu)", i / 3, i % 3);
    HostCall hc(ctx);
    const float* dl = hc.in(lut, n);
    const uint8_t* di = hc.in(bgr, npix * 3);
    uint8_t* dout = hc.out(out_bgr, npix * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_lut_apply(ctx, ctx->stream, dl, size, di, (long)npix, dout));
    return hc.finish();
}

int nct_lut_apply_dev(nct_ctx* ctx, const float* d_lut, int size, const uint8_t* d_bgr, size_t npix, uint8_t* d_out_bgr) {
    NCT_CTX_ENTER();
    NCT_TRY(lut_apply_check(ctx, "lut_apply_dev", d_lut, size, d_bgr, npix, d_out_bgr));
    return nctk_lut_apply(ctx, ctx->stream, d_lut, size, d_bgr, (long)npix, d_out_bgr);
}

}  // extern "C"
