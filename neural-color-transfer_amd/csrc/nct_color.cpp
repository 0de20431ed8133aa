// nct_color.cpp — C-ABI entry points of the colour stage (host-pointer variants used by tests and by integrators that
// want to replace a single seam of transfer_color_single_bds; the fused per-pair path lives in nct_pipeline.cpp).
#include "nct_internal.h"
#include <cstring>


extern "C" {

void nct_params_default(nct_params* p) {
    if (!p) return;
    // Config::Config() (ColorTransfer/Config.h:58-72) — NOT the values quoted in the help strings (main.cu:40-43)
    p->bds_weight = 2.0; p->eps = 0.60; p->nonlocal_weight = 2.0; p->local_weight = 0.125; p->wls_lambda_init = 0.024;
    p->cluster_num = 10; p->k_num = 8; p->patch_size = 3; p->wls_alpha = 1.2;
    p->pm_iters = 10; p->seed = 1;
    p->levels = 5; p->flags = 0;
}

int nct_bgr2lab_u8(nct_ctx* ctx, const uint8_t* bgr, size_t npix, uint8_t* lab) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(bgr && lab && npix > 0, "bgr2lab: bad arguments");
    HostCall hc(ctx);
    const uint8_t* a = hc.in(bgr, npix * 3);
    uint8_t* b = hc.out(lab, npix * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, a, b, npix));
    return hc.finish();
}
int nct_lab2bgr_u8(nct_ctx* ctx, const uint8_t* lab, size_t npix, uint8_t* bgr) { return nct_lab2bgr_u8_form(ctx, lab, npix, bgr, NCT_LAB2BGR_PIECEWISE); }
int nct_lab2bgr_u8_form(nct_ctx* ctx, const uint8_t* lab, size_t npix, uint8_t* bgr, int form) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(bgr && lab && npix > 0, "lab2bgr: bad arguments");
    NCT_REQUIRE(form == NCT_LAB2BGR_CUBE || form == NCT_LAB2BGR_PIECEWISE, "lab2bgr: unknown form %d", form);
    HostCall hc(ctx);
    const uint8_t* a = hc.in(lab, npix * 3);
    uint8_t* b = hc.out(bgr, npix * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_lab2bgr(ctx, ctx->stream, a, b, npix, form));
    return hc.finish();
}
int nct_resize_u8c3(nct_ctx* ctx, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(src && dst && sh > 0 && sw > 0 && dh > 0 && dw > 0, "resize_u8c3: bad arguments");
    HostCall hc(ctx);
    const uint8_t* a = hc.in(src, (size_t)sh * sw * 3);
    uint8_t* b = hc.out(dst, (size_t)dh * dw * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_resize_u8c3(ctx, ctx->stream, a, sh, sw, b, dh, dw));
    return hc.finish();
}
// ---- source region masks (SPEC §6.11): the three steps alone, on host maps
int nct_resize_u8c1(nct_ctx* ctx, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_resize_u8c1_check(ctx, "resize_u8c1", src, sh, sw, dst, dh, dw));
    HostCall hc(ctx);
    const uint8_t* a = hc.in(src, (size_t)sh * sw);
    uint8_t* b = hc.out(dst, (size_t)dh * dw);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_resize_u8c1(ctx, ctx->stream, a, sh, sw, b, dh, dw));
    return hc.finish();
}
int nct_region_mix(nct_ctx* ctx, const double* x, const uint8_t* mask, int h, int w, double* x_out) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(x && mask && x_out, "region_mix: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "region_mix: grid %dx%d out of range", w, h);
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    double* dx = hc.inout(x, x_out, 6 * n);
    const uint8_t* dm = hc.in(mask, n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_region_mix(ctx, ctx->stream, dx, dm, h, w, dx));          // in place, as a level does it
    return hc.finish();
}
int nct_region_compose(nct_ctx* ctx, const uint8_t* s_bgr, const uint8_t* lab_out, const uint8_t* mask, size_t npix, const nct_region_params* region, const nct_params* prm,
                       uint8_t* out_bgr) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_compose_check(ctx, "region_compose", s_bgr, lab_out, mask, npix, region, prm, out_bgr));
    HostCall hc(ctx);
    const uint8_t* ds = hc.in(s_bgr, npix * 3);
    uint8_t* dls = hc.scratch<uint8_t>(npix * 3);
    const uint8_t *dlo = hc.in(lab_out, npix * 3), *dm = hc.in(mask, npix);
    uint8_t* dout = hc.out(out_bgr, npix * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, ds, dls, npix));
    NCT_TRY(nctk_region_compose(ctx, ctx->stream, ds, dls, dlo, dm, npix, region ? region->protect : 0, nct_cube_form(*prm), dout));
    return hc.finish();
}

// ---- reference region masks (SPEC §6.12 rule 2): the pull alone, on host maps
int nct_region_pull(nct_ctx* ctx, const uint8_t* q_mask, int bh, int bw, const uint32_t* ann, const uint32_t* bnn, int ah, int aw, double w_coherence, double w_complete,
                    uint8_t* out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_pull_check(ctx, "region_pull", q_mask, bh, bw, ann, bnn, ah, aw, out));
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    HostCall hc(ctx);
    const uint8_t* dq = hc.in(q_mask, nb);
    uint8_t* dout = hc.out(out, na);
    const uint32_t *da = hc.in(ann, na), *db = hc.in(bnn, nb);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_region_pull(ctx, ctx->stream, dq, bh, bw, da, db, ah, aw, w_coherence, w_complete, dout));
    return hc.finish();
}

int nct_resize_f64c3(nct_ctx* ctx, const double* src, int sh, int sw, double* dst, int dh, int dw) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(src && dst && sh > 0 && sw > 0 && dh > 0 && dw > 0, "resize_f64c3: bad arguments");
    HostCall hc(ctx);
    const double* a = hc.in(src, (size_t)sh * sw * 3);
    double* b = hc.out(dst, (size_t)dh * dw * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_resize_f64c3(ctx, ctx->stream, a, sh, sw, b, dh, dw));
    return hc.finish();
}

int nct_cluster_features(nct_ctx* ctx, const float* feat_chw, int C, int h, int w, int K, int iters, uint64_t seed, int* labels, int* nlabels) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(feat_chw && labels && nlabels && h > 0 && w > 0 && (C & 3) == 0, "cluster_features: bad arguments");
    const int n = h * w;
    HostCall hc(ctx);
    const float* t = hc.in(feat_chw, (size_t)C * n);
    float *f = hc.scratch<float>((size_t)C * n), *fn = hc.scratch<float>((size_t)C * n);
    int *lab = hc.out(labels, n), *nl = hc.out(nlabels, 1);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_chw_to_hwc(ctx, ctx->stream, t, f, C, n));
    NCT_TRY(nctk_normalize(ctx, ctx->stream, f, fn, nullptr, C, n));          // main.cu:139-165 (per-pixel L2 normalise, HWC)
    NCT_TRY(nctk_kmeans_labels(ctx, ctx->stream, fn, n, C, K, iters, seed, lab, nl));
    return hc.finish();
}

int nct_knn_graph(nct_ctx* ctx, const uint8_t* lab_u8, int h, int w, const int* labels, int lh, int lw, int nlabels, int samples, int k,
                  int* knn_id, double* knn_w) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(lab_u8 && labels && knn_id && knn_w && h > 0 && w > 0 && lh > 0 && lw > 0 && samples > 0, "knn_graph: bad arguments");
    NCT_REQUIRE(k == 8, "knn_graph: only k=8 is supported (Config.h:68), got %d", k);
    const int n = h * w;
    HostCall hc(ctx);
    const uint8_t* l = hc.in(lab_u8, (size_t)n * 3);
    const int* lb = hc.in(labels, (size_t)lh * lw);
    int* id = hc.out(knn_id, (size_t)n * 8);
    double* kw = hc.out(knn_w, (size_t)n * 8);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_knn_graph(ctx, ctx->stream, l, h, w, lb, lh, lw, nlabels, nullptr, samples, id, kw));
    return hc.finish();
}

int nct_local_color_transfer(nct_ctx* ctx, const float* err, const uint8_t* s_bgr_level, const uint8_t* g_bgr_level, const uint8_t* s_bgr_full,
                             const int* knn_id, const double* knn_w, int layer, int h, int w, int H, int W, const nct_params* prm,
                             uint8_t* out_bgr_full, nct_color_stages* stages) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(err && s_bgr_level && g_bgr_level && s_bgr_full && knn_id && knn_w && prm && out_bgr_full, "local_color_transfer: null pointer");
    NCT_REQUIRE(h > 0 && w > 0 && H >= h && W >= w && layer >= 0 && layer <= 4, "local_color_transfer: bad geometry");
    NCT_TRY(nct_params_check(ctx, "local_color_transfer", *prm));
    const size_t n = (size_t)h * w, N = (size_t)H * W;
    HostCall hc(ctx);
    const float* derr = hc.in(err, n);
    const uint8_t *sl = hc.in(s_bgr_level, n * 3), *gl = hc.in(g_bgr_level, n * 3), *sf = hc.in(s_bgr_full, N * 3);
    uint8_t *slab = hc.scratch<uint8_t>(n * 3), *glab = hc.scratch<uint8_t>(n * 3), *sflab = hc.scratch<uint8_t>(N * 3), *olab = hc.scratch<uint8_t>(N * 3), *obgr = hc.out(out_bgr_full, N * 3);
    const int* id = hc.in(knn_id, n * 8);
    const double* kw = hc.in(knn_w, n * 8);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, sl, slab, n));          // main.cu:351-352
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, gl, glab, n));          // main.cu:370-371
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, sf, sflab, N));         // ColorTransfer.h:58
    const nct_color_params cp = nct_color_params_of(*prm);
    nct_color_debug dbg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (stages) { dbg.ab_local = stages->ab_local; dbg.ab_nonlocal = stages->ab_nonlocal; dbg.ab_up = stages->ab_up; dbg.rough = stages->roughness;
                  dbg.ab_wls = stages->ab_wls; dbg.cg_iters = stages->cg_iters; dbg.wls_iters = stages->wls_iters; }
    {
        nct_color_bufs cb;                                         // T1 .. S1 (its graph part built inside), then the finish on the working grid
        NCT_TRY(nctk_color_nonlocal(ctx, ctx->stream, derr, slab, glab, id, kw, layer, h, w, H, W, cp, cb, stages ? &dbg : nullptr));
        NCT_TRY(nctk_color_finish(ctx, ctx->stream, cb.x, h, w, H, W, sflab, H, W, cp, olab, stages ? &dbg : nullptr));
    }
    NCT_TRY(nctk_lab2bgr(ctx, ctx->stream, olab, obgr, N, nct_cube_form(*prm)));        // ColorTransfer.cpp:1469
    return hc.finish();
}

// the finish alone (SPEC §6.1): U1 / roughness / S2 / A1 of S1's coefficients onto s_bgr_full, which may be larger than the working size
int nct_color_finish(nct_ctx* ctx, const double* ab, int h, int w, int work_h, int work_w, const uint8_t* s_bgr_full, int H, int W, const nct_params* prm,
                     uint8_t* out_bgr_full, nct_color_stages* stages) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(ab && s_bgr_full && prm && out_bgr_full, "color_finish: null pointer");
    NCT_REQUIRE(h > 0 && w > 0 && work_h >= h && work_w >= w && H >= h && W >= w, "color_finish: bad geometry (level %dx%d, working %dx%d, target %dx%d)", w, h, work_w, work_h, W, H);
    NCT_REQUIRE(H <= NCT_FINISH_MAX_SIDE && W <= NCT_FINISH_MAX_SIDE && (long long)H * W <= NCT_FINISH_MAX_PIXELS, "color_finish: target %dx%d above 16384 per side or 2^26 pixels", W, H);
    NCT_TRY(nct_params_check(ctx, "color_finish", *prm));
    const size_t n = (size_t)h * w, N = (size_t)H * W;
    HostCall hc(ctx);
    const double* x = hc.in(ab, 6 * n);
    const uint8_t* sf = hc.in(s_bgr_full, N * 3);
    uint8_t *sflab = hc.scratch<uint8_t>(N * 3), *olab = hc.scratch<uint8_t>(N * 3), *obgr = hc.out(out_bgr_full, N * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, sf, sflab, N));
    const nct_color_params cp = nct_color_params_of(*prm);
    nct_color_debug dbg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (stages) { dbg.ab_up = stages->ab_up; dbg.rough = stages->roughness; dbg.ab_wls = stages->ab_wls; dbg.wls_iters = stages->wls_iters; }
    ctx->wls_split = (prm->flags & NCT_FLAG_LATENCY) ? 1 : 0;
    NCT_TRY(nctk_color_finish(ctx, ctx->stream, x, h, w, work_h, work_w, sflab, H, W, cp, olab, stages ? &dbg : nullptr));
    NCT_TRY(nctk_lab2bgr(ctx, ctx->stream, olab, obgr, N, nct_cube_form(*prm)));
    return hc.finish();
}

// ---- the upsampling finish alone, on host pointers, in its four forms (k_finish_up.hip): the working-size S2 output upsampled and applied to the original source in one
// kernel (SPEC §6.8); is_guided: with joint-bilateral weights (SPEC §6.10); mask non-null: with the compose in the pass (SPEC §6.13 rule 4; mask NULL is the unmasked call)
static int finish_up_host(nct_ctx* ctx, bool is_guided, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, int H, int W, const uint8_t* mask,
                          const nct_region_params* region, const nct_guided_params* guided, const nct_params* prm, uint8_t* out_bgr_full) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm && (guided || !is_guided), "%s: null pointer", nct_finish_up_name(is_guided, mask != nullptr));
    NCT_TRY(nct_params_check(ctx, nct_finish_up_name(is_guided, mask != nullptr), *prm));
    const nct_finish_up host{s_bgr_full, H, W, out_bgr_full, nct_cube_form(*prm), is_guided ? guided->sigma : 0.0, mask, region ? region->protect : 0};
    NCT_TRY(nctk_finish_up_check(ctx, is_guided, ab_wls, lab_work, h, w, host));      // before anything is reserved
    const size_t n = (size_t)h * w, N = (size_t)H * W;
    HostCall hc(ctx);
    const double* x = hc.in(ab_wls, 6 * n);
    const uint8_t* lw = is_guided ? hc.in(lab_work, n * 3) : nullptr;
    nct_finish_up up = host;                                                          // the same call on the device copies
    up.s_bgr = hc.in(s_bgr_full, N * 3); up.mask = hc.in(mask, N); up.out_bgr = hc.out(out_bgr_full, N * 3);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_finish_up(ctx, ctx->stream, x, lw, h, w, up));
    return hc.finish();
}

int nct_color_finish_upsample(nct_ctx* ctx, const double* ab_wls, int h, int w, const uint8_t* s_bgr_full, int H, int W, const nct_params* prm, uint8_t* out_bgr_full) {
    return finish_up_host(ctx, false, ab_wls, nullptr, h, w, s_bgr_full, H, W, nullptr, nullptr, nullptr, prm, out_bgr_full);
}

// ---- the guided finish (SPEC §6.10): the upsampling finish with joint-bilateral weights (k_finish_up.hip: k_finish_guided)
void nct_guided_params_default(nct_guided_params* p) {
    if (!p) return;
    p->sigma = 10.0;
}

// the modifier of a context: non-null = every upsampling finish behind a working-size finish (finish_level, nct_pipeline.cpp) runs guided from the next one enqueued on
int nct_set_finish_guided(nct_ctx* ctx, const nct_guided_params* guided) {
    if (!ctx) return NCT_ERR_INVALID;
    NCT_REQUIRE(!guided || nct_guided_sigma_ok(guided->sigma), "set_finish_guided: sigma must be finite and > 0, and so must its square (got %g)", guided->sigma);
    ctx->guided_sigma = guided ? guided->sigma : 0.0;
    return NCT_OK;
}

int nct_color_finish_guided(nct_ctx* ctx, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, int H, int W, const nct_guided_params* guided,
                            const nct_params* prm, uint8_t* out_bgr_full) {
    return finish_up_host(ctx, true, ab_wls, lab_work, h, w, s_bgr_full, H, W, nullptr, nullptr, guided, prm, out_bgr_full);
}

int nct_color_finish_upsample_region(nct_ctx* ctx, const double* ab_wls, int h, int w, const uint8_t* s_bgr_full, int H, int W, const uint8_t* mask, const nct_region_params* region,
                                     const nct_params* prm, uint8_t* out_bgr_full) {
    return finish_up_host(ctx, false, ab_wls, nullptr, h, w, s_bgr_full, H, W, mask, region, nullptr, prm, out_bgr_full);
}

int nct_color_finish_guided_region(nct_ctx* ctx, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, int H, int W, const uint8_t* mask,
                                   const nct_region_params* region, const nct_guided_params* guided, const nct_params* prm, uint8_t* out_bgr_full) {
    return finish_up_host(ctx, true, ab_wls, lab_work, h, w, s_bgr_full, H, W, mask, region, guided, prm, out_bgr_full);
}

}  // extern "C"
