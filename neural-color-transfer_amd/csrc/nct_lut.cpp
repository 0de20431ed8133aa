// nct_lut.cpp — C ABI of the 3D colour look-up tables (SPEC §6.6): fit from a (source, result) pair, apply, on host and on device pointers; the shot
// accumulator and the apply on 16-bit pixels (SPEC §6.20).
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

// ---- the shot accumulator (SPEC §6.20): rule 3's sums over every pixel offered between begin and end, owned by the context like a sequence's state. kept: the
// device counter the masked splats add to; the pixels of unmasked adds are counted on the host
struct lut_accum {
    int N = 0;
    DevBuf<uint64_t> W, kept; DevBuf<int64_t> R;
    uint64_t adds = 0, offered = 0, kept_unmasked = 0, masked_adds = 0;
};
void nct_lut_accum_free(nct_ctx* ctx) { delete (lut_accum*)ctx->lut_accum; ctx->lut_accum = nullptr; }

#define NCT_LUT_ACCUM_OPEN(what) lut_accum* A = (lut_accum*)ctx->lut_accum; \
    if (!A) return ctx->fail(NCT_ERR_STATE, "%s: no accumulator is open on this context (nct_lut_accum_begin first)", what)

static int lut_accum_add_check(nct_ctx* ctx, const char* what, const lut_accum* A, const void* src, const void* res, size_t npix) {
    NCT_REQUIRE(src && res, "%s: null pointer", what);
    NCT_REQUIRE(npix >= 1 && npix <= (size_t)NCT_LUT_MAX_PIXELS, "%s: the number of pixels must be in [1, 2^26] (got %zu)", what, npix);
    NCT_REQUIRE(A->offered + npix <= NCT_LUT_ACCUM_MAX_PIXELS, "%s: an accumulator takes at most 2^30 pixels (%llu offered so far, %zu more asked for)", what,
                (unsigned long long)A->offered, npix);
    return NCT_OK;
}
// one splat launch into the owned sums, nothing zeroed; the host-side counts move once it is enqueued
static int lut_accum_splat(nct_ctx* ctx, lut_accum* A, const uint8_t* d_src, const uint8_t* d_res, const uint8_t* d_mask, size_t npix) {
    if (d_mask) NCT_TRY(nctk_lut_splat_masked(ctx, ctx->stream, d_src, d_res, d_mask, (long)npix, A->N, A->W, A->R, A->kept, true));
    else NCT_TRY(nctk_lut_splat(ctx, ctx->stream, d_src, d_res, (long)npix, A->N, A->W, A->R, true));
    ++A->adds; A->offered += npix;
    if (d_mask) ++A->masked_adds; else A->kept_unmasked += npix;
    return NCT_OK;
}
// the kept pixels so far: the host's count, and with masked adds the device counter, which is waited for
static int lut_accum_kept(nct_ctx* ctx, const lut_accum* A, uint64_t* out) {
    uint64_t masked = 0;
    if (A->masked_adds) { NCT_D2H(&masked, A->kept, sizeof masked); NCT_SYNC(); }
    *out = A->kept_unmasked + masked;
    return NCT_OK;
}
static int lut_accum_solve_check(nct_ctx* ctx, const char* what, const lut_accum* A, double lambda, const void* lut_out) {
    NCT_REQUIRE(lut_out, "%s: null pointer", what);
    NCT_REQUIRE(std::isfinite(lambda) && lambda > 0.0, "%s: lambda must be finite and greater than 0 (got %g)", what, lambda);
    uint64_t kept = 0;
    NCT_TRY(lut_accum_kept(ctx, A, &kept));
    NCT_REQUIRE(kept > 0, "%s: the accumulator keeps no pixel (%llu offered in %llu adds)", what, (unsigned long long)A->offered, (unsigned long long)A->adds);
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

// SPEC §6.20: the table on 16-bit pixels
int nct_lut_apply_u16(nct_ctx* ctx, const float* lut, int size, const uint16_t* bgr16, size_t npix, uint16_t* out_bgr16) {
    NCT_CTX_ENTER();
    NCT_TRY(lut_apply_check(ctx, "lut_apply_u16", lut, size, bgr16, npix, out_bgr16));
    const size_t n = (size_t)size * size * size * 3;
    for (size_t i = 0; i < n; ++i) NCT_REQUIRE(std::isfinite(lut[i]), "lut_apply_u16: the table has a non-finite entry (node %zu, channel %zu)", i / 3, i % 3);
    HostCall hc(ctx);
    const float* dl = hc.in(lut, n);
    const uint16_t* di = hc.in(bgr16, npix * 3);
    uint16_t* dout = hc.out(out_bgr16, npix * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_lut_apply16(ctx, ctx->stream, dl, size, di, (long)npix, dout));
    return hc.finish();
}

int nct_lut_apply_u16_dev(nct_ctx* ctx, const float* d_lut, int size, const uint16_t* d_bgr16, size_t npix, uint16_t* d_out_bgr16) {
    NCT_CTX_ENTER();
    NCT_TRY(lut_apply_check(ctx, "lut_apply_u16_dev", d_lut, size, d_bgr16, npix, d_out_bgr16));
    return nctk_lut_apply16(ctx, ctx->stream, d_lut, size, d_bgr16, (long)npix, d_out_bgr16);
}

// SPEC §6.20: the shot accumulator
int nct_lut_accum_begin(nct_ctx* ctx, int size) {
    NCT_CTX_ENTER();
    if (ctx->lut_accum) return ctx->fail(NCT_ERR_STATE, "lut_accum_begin: an accumulator is open on this context (nct_lut_accum_end first)");
    NCT_REQUIRE(nct_lut_size_ok(size), "lut_accum_begin: the lattice size must be one of 3, 5, 9, 17, 33, 65 (got %d)", size);
    const size_t n3 = (size_t)size * size * size;
    lut_accum* A = new lut_accum();
    A->N = size;
    int rc = A->W.alloc(ctx, n3) && A->R.alloc(ctx, n3 * 3) && A->kept.alloc(ctx, 1) ? NCT_OK : NCT_ERR_HIP;
    if (!rc) rc = nctk_lut_accum_zero(ctx, ctx->stream, size, A->W, A->R, A->kept);
    if (rc) { delete A; return rc; }
    ctx->lut_accum = A;
    return NCT_OK;
}

int nct_lut_accum_add(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, const uint8_t* mask, size_t npix) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_add");
    NCT_TRY(lut_accum_add_check(ctx, "lut_accum_add", A, src_bgr, res_bgr, npix));
    HostCall hc(ctx);
    const uint8_t *ds = hc.in(src_bgr, npix * 3), *dr = hc.in(res_bgr, npix * 3), *dm = hc.in(mask, npix);
    NCT_TRY(hc.ready());
    NCT_TRY(lut_accum_splat(ctx, A, ds, dr, dm, npix));
    return hc.finish();
}

int nct_lut_accum_add_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, const uint8_t* d_mask, size_t npix) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_add_dev");
    NCT_TRY(lut_accum_add_check(ctx, "lut_accum_add_dev", A, d_src_bgr, d_res_bgr, npix));
    return lut_accum_splat(ctx, A, d_src_bgr, d_res_bgr, d_mask, npix);
}

// the images nct_pair_fit_lut would read, from where they lie on the device
int nct_lut_accum_add_run(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_add_run");
    nct_lut_images im;
    if (!nct_pair_lut_images(ctx, &im)) return ctx->fail(NCT_ERR_STATE, "lut_accum_add_run: no finished run on this context (nct_pair_run first)");
    NCT_TRY(lut_accum_add_check(ctx, "lut_accum_add_run", A, im.src, im.res, im.npix));
    return lut_accum_splat(ctx, A, im.src, im.res, im.mask, im.npix);
}

int nct_lut_accum_info(nct_ctx* ctx, int* size, uint64_t* adds, uint64_t* pixels_offered, uint64_t* pixels_kept) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_info");
    if (pixels_kept) NCT_TRY(lut_accum_kept(ctx, A, pixels_kept));
    if (size) *size = A->N;
    if (adds) *adds = A->adds;
    if (pixels_offered) *pixels_offered = A->offered;
    return NCT_OK;
}

int nct_lut_accum_solve(nct_ctx* ctx, double lambda, float* lut_out, nct_lut_stages* stages) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_solve");
    NCT_TRY(lut_accum_solve_check(ctx, "lut_accum_solve", A, lambda, lut_out));
    const size_t n3 = (size_t)A->N * A->N * A->N;
    HostCall hc(ctx);
    float* dl = hc.out(lut_out, n3 * 3);
    double* d = hc.scratch<double>(n3 * 3);
    // W and R come down from the owned sums, which the solve only reads
    if (stages) { hc.get(stages->weight, (uint64_t*)A->W, n3); hc.get(stages->resid, (int64_t*)A->R, n3 * 3); hc.get(stages->disp, d, n3 * 3); }
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_lut_solve(ctx, ctx->stream, A->W, A->R, A->N, lambda, d));
    NCT_TRY(nctk_lut_table(ctx, ctx->stream, d, A->N, dl));
    return hc.finish();
}

int nct_lut_accum_solve_dev(nct_ctx* ctx, double lambda, float* d_lut_out, nct_lut_stages* d_stages) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_solve_dev");
    NCT_TRY(lut_accum_solve_check(ctx, "lut_accum_solve_dev", A, lambda, d_lut_out));
    const size_t n3 = (size_t)A->N * A->N * A->N;
    DevBuf<double> d;
    double* D = d_stages && d_stages->disp ? d_stages->disp : nullptr;
    if (!D) { if (!d.alloc(ctx, n3 * 3)) return NCT_ERR_HIP; D = d; }
    if (d_stages && d_stages->weight) NCT_HIP(hipMemcpyAsync(d_stages->weight, A->W, n3 * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    if (d_stages && d_stages->resid) NCT_HIP(hipMemcpyAsync(d_stages->resid, A->R, n3 * 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, ctx->stream));
    NCT_TRY(nctk_lut_solve(ctx, ctx->stream, A->W, A->R, A->N, lambda, D));
    return nctk_lut_table(ctx, ctx->stream, D, A->N, d_lut_out);
}

int nct_lut_accum_end(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    NCT_LUT_ACCUM_OPEN("lut_accum_end");
    nct_lut_accum_free(ctx);
    return NCT_OK;
}

}  // extern "C"
