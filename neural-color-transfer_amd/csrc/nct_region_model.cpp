// nct_region_model.cpp — region models (SPEC §6.17): what a selection from strokes learnt, kept so that the object can be found again on another image. The model is a
// host object without a context: the tap and the kept seed rows of §6.16 rule 3, inside and outside, as int16. Applying it to an image is the chain VGG19 forward to the
// tap -> quantise -> score against the model's rows -> re-find (resize to the image, fused with a carried matte where the score is not confident) -> snap passes, on
// device pointers. Kernel of the re-find: k_region_refind.hip; the others are region selection's. Every transient is an arena block that goes back in stream order.
// An open sequence may hold a model's rows on the device (nct_seq_set_region_model): every full frame then re-finds from the tap of its own forward (seq_refind_step,
// called by nct_pipeline.cpp's run behind the forward), with the tracked matte as the prior.
#include "nct_pipeline.h"
#include <algorithm>

#define NCT_MODEL_MAX_ROWS 65536                 // nct_region_score's limit per class

struct nct_region_model { int tap = 0, C = 0; std::vector<int16_t> in, out; };   // rows [n][C] in the raster order of §6.16 rule 3, image after image

void nct_region_refind_params_default(nct_region_refind_params* p) {
    if (!p) return;
    p->sharpness = 1024; p->floor_permille = 700; p->margin = 32; p->snap_iters = 1;
    nct_region_snap_params_default(&p->snap);
}

// §6.16 rules 1-3 on a host image and its strokes: the kept rows, inside then outside, into host vectors
static int model_rows_of(nct_ctx* ctx, const char* who, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params, int* tap,
                         std::vector<int16_t>& rows_in, std::vector<int16_t>& rows_out) {
    nct_region_select_params p;
    NCT_TRY(select_check(ctx, who, src_bgr, h, w, strokes, params, /* no matte is written */ src_bgr, &p));
    const size_t N = (size_t)h * w;
    const int C = kTapC[p.tap - 1];
    select_rows r;                                               // outlives the call's wait: its rows come down in finish()
    HostCall hc(ctx);
    const uint8_t *ds = hc.in(src_bgr, N * 3), *dt = hc.in(strokes, N);
    NCT_TRY(hc.ready());
    NCT_TRY(select_seed_rows(ctx, who, ds, h, w, dt, p, nullptr, false, r));
    rows_in.resize((size_t)r.k_in * C); rows_out.resize((size_t)r.k_out * C);
    hc.get(rows_in.data(), (const int16_t*)r.seeds, rows_in.size());
    if (r.k_out) hc.get(rows_out.data(), (const int16_t*)r.seeds + rows_in.size(), rows_out.size());
    *tap = p.tap;
    return hc.finish();
}

static int refind_params_check(nct_ctx* ctx, const char* who, const nct_region_refind_params* params, nct_region_refind_params* p) {
    if (params) *p = *params; else nct_region_refind_params_default(p);
    NCT_REQUIRE(p->sharpness >= 1 && p->sharpness <= 65536, "%s: sharpness must be in [1, 65536] (got %d)", who, p->sharpness);
    NCT_REQUIRE(p->floor_permille >= 0 && p->floor_permille <= 1000, "%s: floor_permille must be in [0, 1000] (got %d)", who, p->floor_permille);
    NCT_REQUIRE(p->margin >= 0 && p->margin <= 128, "%s: margin must be in [0, 128] (got %d)", who, p->margin);
    NCT_REQUIRE(p->snap_iters >= 0 && p->snap_iters <= 8, "%s: snap_iters must be in [0, 8] (got %d)", who, p->snap_iters);
    return nct_region_snap_params_check(ctx, who, &p->snap);
}

// the arguments of nct_region_model_apply[_dev] and of what is built on it; on success *p holds the parameters in force
static int apply_check(nct_ctx* ctx, const char* who, const nct_region_model* model, const void* src_bgr, int h, int w, const nct_region_refind_params* params, const void* mask_out,
                       nct_region_refind_params* p) {
    NCT_REQUIRE(model, "%s: null model", who);
    NCT_REQUIRE(src_bgr, "%s: null src_bgr", who);
    NCT_REQUIRE(mask_out, "%s: null mask_out", who);
    NCT_REQUIRE(h >= 17 && h <= 4000, "%s: h must be in [17, 4000] (got %d)", who, h);
    NCT_REQUIRE(w >= 17 && w <= 4000, "%s: w must be in [17, 4000] (got %d)", who, w);
    NCT_TRY(refind_params_check(ctx, who, params, p));
    if (nct_vgg19_weights_info(ctx, nullptr, nullptr, nullptr) != NCT_OK)
        return ctx->fail(NCT_ERR_STATE, "%s: VGG19 weights not loaded (nct_vgg19_load_caffemodel / _load_raw)", who);
    return NCT_OK;
}

// SPEC §6.17 rules A1-A4 on device pointers, checked arguments; d_prior nullable. st (nullable): HOST arrays for the stages, each copied and waited for as it is made.
// The one wait of the plain chain is for the model's rows
static int apply_enqueue(nct_ctx* ctx, const nct_region_model* M, const uint8_t* d_src, int h, int w, const uint8_t* d_prior, const nct_region_refind_params& p, uint8_t* d_out,
                         const nct_region_apply_stages* st) {
    hipStream_t s = ctx->stream;
    const int tap = M->tap, C = M->C, ht = ((h - 1) >> (tap - 1)) + 1, wt = ((w - 1) >> (tap - 1)) + 1, cells = ht * wt;
    const int n_in = (int)(M->in.size() / C), n_out = (int)(M->out.size() / C);
    const size_t N = (size_t)h * w;
    // the model's rows go up first and are waited for, while the stream is still short: the model may be changed or freed as soon as the call returns
    DevBuf<int16_t> rows;
    if (!rows.alloc(ctx, M->in.size() + M->out.size())) return NCT_ERR_HIP;
    NCT_H2D(rows, M->in.data(), sizeof(int16_t) * M->in.size());
    if (n_out) NCT_H2D((int16_t*)rows + M->in.size(), M->out.data(), sizeof(int16_t) * M->out.size());
    NCT_SYNC();
    // A1
    DevBuf<int16_t> q;
    if (!q.alloc(ctx, (size_t)cells * C)) return NCT_ERR_HIP;
    NCT_TRY(select_quantised_tap(ctx, s, d_src, h, w, tap, q));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->q, q, (size_t)cells * C));
    // A2: no cell of this image is a seed cell, nothing is overwritten
    DevBuf<uint8_t> m;
    if (!m.alloc(ctx, cells)) return NCT_ERR_HIP;
    NCT_TRY(nctk_region_score(ctx, s, q, cells, C, rows, n_in, (int16_t*)rows + M->in.size(), n_out, p.sharpness, p.floor_permille, nullptr, m));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->score, m, (size_t)cells));
    // A3 and A4: every snap pass runs out of place between d_out and one block of scratch; the re-found matte goes where the last pass ends in d_out
    DevBuf<uint8_t> alt, lab;
    if (p.snap_iters > 0) {
        if (!alt.alloc(ctx, N) || !lab.alloc(ctx, N * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, d_src, lab, N));
    }
    uint8_t *cur = (p.snap_iters & 1) ? (uint8_t*)alt : d_out, *oth = (p.snap_iters & 1) ? d_out : (uint8_t*)alt;
    NCT_TRY(nctk_region_refind(ctx, s, m, ht, wt, d_prior, h, w, p.margin, cur));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->refound, cur, N));
    for (int it = 0; it < p.snap_iters; ++it) {
        NCT_TRY(nctk_region_snap(ctx, s, cur, lab, h, w, &p.snap, oth));
        std::swap(cur, oth);
    }
    return NCT_OK;
}

int seq_refind_step(nct_ctx* ctx, hipStream_t s, pair_state* P, seq_state* q, const float* tap_hwc, const uint8_t* lab_work) {
    const int tap = q->model_tap, C = q->model_C, h = P->sh, w = P->sw, ht = ((h - 1) >> (tap - 1)) + 1, wt = ((w - 1) >> (tap - 1)) + 1, cells = ht * wt;
    const bool full = q->target() != nullptr;
    const int H = full ? q->full.H : h, W = full ? q->full.W : w;
    const size_t N = (size_t)H * W;
    const nct_region_refind_params& p = q->model_p;
    // A1 and A2 on the tap the frame's forward wrote
    DevBuf<int16_t> rows;
    DevBuf<uint8_t> m;
    if (!rows.alloc(ctx, (size_t)cells * C) || !m.alloc(ctx, cells)) return NCT_ERR_HIP;
    NCT_TRY(nctk_feat_quantize(ctx, s, tap_hwc, rows, C, cells));
    NCT_TRY(nctk_region_score(ctx, s, rows, cells, C, q->model_rows, q->model_n_in, (int16_t*)q->model_rows + (size_t)q->model_n_in * C, q->model_n_out, p.sharpness, p.floor_permille, nullptr, m));
    // rule S3: the matte the track step left is the prior, unless the sequence has no state — the old shot's matte is not evidence
    const bool had = P->mask != nullptr, prior = had && q->frames > 0;
    if (!P->mask.reserve(ctx, (size_t)h * w)) return NCT_ERR_HIP;
    if (full && !P->full_mask.reserve(ctx, N)) return NCT_ERR_HIP;
    DevBuf<uint8_t>& matte = full ? P->full_mask : P->mask;
    if ((prior || p.snap_iters > 0) && !q->matte_alt.reserve(ctx, N)) return NCT_ERR_HIP;
    // rule S4: from the working-size tap grid straight to the size frames arrive, out of place where there is a prior; the two matte blocks then change places
    if (prior) {
        NCT_TRY(nctk_region_refind(ctx, s, m, ht, wt, matte, H, W, p.margin, q->matte_alt));
        matte.swap(q->matte_alt);
    } else NCT_TRY(nctk_region_refind(ctx, s, m, ht, wt, nullptr, H, W, p.margin, matte));
    // rule S5: the model's snap passes, then the shrink of a full-resolution sequence
    NCT_TRY(seq_matte_snap(ctx, s, P, q, lab_work, p.snap, p.snap_iters));
    P->protect = q->model_protect;
    if (!had) { q->matte_fresh = false; q->matte_age = 0; }      // this frame is the new matte's own
    return NCT_OK;
}

static inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) { return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; }

extern "C" {

int nct_region_model_fit(nct_ctx* ctx, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params, nct_region_model** model) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(model, "region_model_fit: null model");
    nct_region_model* M = new nct_region_model();
    const int rc = model_rows_of(ctx, "region_model_fit", src_bgr, h, w, strokes, params, &M->tap, M->in, M->out);
    if (rc) { delete M; return rc; }
    M->C = kTapC[M->tap - 1];
    *model = M;
    return NCT_OK;
}

int nct_region_model_add(nct_ctx* ctx, nct_region_model* model, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(model, "region_model_add: null model");
    nct_region_select_params dflt;
    nct_region_select_params_default(&dflt);
    const int want = params ? params->tap : dflt.tap;
    NCT_REQUIRE(want < 1 || want > 5 || want == model->tap, "region_model_add: tap %d is not the model's tap %d", want, model->tap);
    int tap = 0;
    std::vector<int16_t> in, out;
    NCT_TRY(model_rows_of(ctx, "region_model_add", src_bgr, h, w, strokes, params, &tap, in, out));
    const size_t C = (size_t)model->C, n_in = (model->in.size() + in.size()) / C, n_out = (model->out.size() + out.size()) / C;
    NCT_REQUIRE(n_in <= NCT_MODEL_MAX_ROWS, "region_model_add: the model would hold %zu inside rows (at most %d)", n_in, NCT_MODEL_MAX_ROWS);
    NCT_REQUIRE(n_out <= NCT_MODEL_MAX_ROWS, "region_model_add: the model would hold %zu outside rows (at most %d)", n_out, NCT_MODEL_MAX_ROWS);
    model->in.reserve(model->in.size() + in.size()); model->out.reserve(model->out.size() + out.size());   // both grow, or neither
    model->in.insert(model->in.end(), in.begin(), in.end());
    model->out.insert(model->out.end(), out.begin(), out.end());
    return NCT_OK;
}

int nct_region_model_info(const nct_region_model* model, int* tap, int* C, int* n_in, int* n_out) {
    if (!model) { nct_set_ctxless_error("region_model_info: null model"); return NCT_ERR_INVALID; }
    if (tap) *tap = model->tap;
    if (C) *C = model->C;
    if (n_in) *n_in = (int)(model->in.size() / model->C);
    if (n_out) *n_out = (int)(model->out.size() / model->C);
    return NCT_OK;
}

int nct_region_model_rows(const nct_region_model* model, const int16_t** rows_in, const int16_t** rows_out) {
    if (!model) { nct_set_ctxless_error("region_model_rows: null model"); return NCT_ERR_INVALID; }
    if (rows_in) *rows_in = model->in.data();
    if (rows_out) *rows_out = model->out.empty() ? nullptr : model->out.data();
    return NCT_OK;
}

int nct_region_model_from_rows(int tap, int C, const int16_t* rows_in, int n_in, const int16_t* rows_out, int n_out, nct_region_model** model) {
    char msg[160];
    const char* why = nullptr;
    if (!model) why = "region_model_from_rows: null model";
    else if (tap < 1 || tap > 5) { snprintf(msg, sizeof msg, "region_model_from_rows: tap must be in [1, 5] (got %d)", tap); why = msg; }
    else if (C != kTapC[tap - 1]) { snprintf(msg, sizeof msg, "region_model_from_rows: C must be %d at tap %d (got %d)", kTapC[tap - 1], tap, C); why = msg; }
    else if (n_in < 1 || n_in > NCT_MODEL_MAX_ROWS) { snprintf(msg, sizeof msg, "region_model_from_rows: n_in must be in [1, %d] (got %d)", NCT_MODEL_MAX_ROWS, n_in); why = msg; }
    else if (n_out < 0 || n_out > NCT_MODEL_MAX_ROWS) { snprintf(msg, sizeof msg, "region_model_from_rows: n_out must be in [0, %d] (got %d)", NCT_MODEL_MAX_ROWS, n_out); why = msg; }
    else if (!rows_in) why = "region_model_from_rows: null rows_in";
    else if (n_out > 0 && !rows_out) why = "region_model_from_rows: null rows_out with n_out > 0";
    if (why) { nct_set_ctxless_error(why); return NCT_ERR_INVALID; }
    nct_region_model* M = new nct_region_model();
    M->tap = tap; M->C = C;
    M->in.assign(rows_in, rows_in + (size_t)n_in * C);
    if (n_out) M->out.assign(rows_out, rows_out + (size_t)n_out * C);
    *model = M;
    return NCT_OK;
}

void nct_region_model_free(nct_region_model* model) { delete model; }

// R1-R3 alone on host arrays: the score and the prior up, one k_region_refind launch, the matte down
int nct_region_refind(nct_ctx* ctx, const uint8_t* score, int ht, int wt, const uint8_t* prior, int H, int W, int margin, uint8_t* out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_refind_check(ctx, "region_refind", score, ht, wt, H, W, margin, out));
    const size_t N = (size_t)H * W, n = (size_t)ht * wt;
    HostCall hc(ctx);
    const uint8_t* dm = hc.in(score, n);
    uint8_t* dout = hc.out(out, N);
    const uint8_t* dp = hc.in(prior, N);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_region_refind(ctx, ctx->stream, dm, ht, wt, dp, H, W, margin, dout));
    return hc.finish();
}

int nct_region_refind_dev(nct_ctx* ctx, const uint8_t* d_score, int ht, int wt, const uint8_t* d_prior, int H, int W, int margin, uint8_t* d_out) {
    NCT_CTX_ENTER();
    return nctk_region_refind(ctx, ctx->stream, d_score, ht, wt, d_prior, H, W, margin, d_out);
}

// measurement hook: the mean device time of one k_region_refind launch, between two events on the library's stream
int nct_region_refind_bench(nct_ctx* ctx, const uint8_t* d_score, int ht, int wt, const uint8_t* d_prior, int H, int W, int margin, uint8_t* d_out, int reps, float* kernel_ms) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(kernel_ms, "region_refind_bench: null kernel_ms");
    NCT_REQUIRE(reps >= 1 && reps <= 1000, "region_refind_bench: reps must be in [1, 1000] (got %d)", reps);
    NCT_TRY(nctk_region_refind(ctx, ctx->stream, d_score, ht, wt, d_prior, H, W, margin, d_out));   // warm-up
    NCT_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < reps; ++r) NCT_TRY(nctk_region_refind(ctx, ctx->stream, d_score, ht, wt, d_prior, H, W, margin, d_out));
    NCT_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    NCT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    NCT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *kernel_ms = ms / reps;
    return NCT_OK;
}

int nct_region_model_apply(nct_ctx* ctx, const nct_region_model* model, const uint8_t* src_bgr, int h, int w, const uint8_t* prior, const nct_region_refind_params* params,
                           uint8_t* mask_out, const nct_region_apply_stages* stages) {
    NCT_CTX_ENTER();
    nct_region_refind_params p;
    NCT_TRY(apply_check(ctx, "region_model_apply", model, src_bgr, h, w, params, mask_out, &p));
    const size_t N = (size_t)h * w;
    HostCall hc(ctx);
    const uint8_t* ds = hc.in(src_bgr, N * 3);
    uint8_t* dm = hc.out(mask_out, N);
    const uint8_t* dp = hc.in(prior, N);
    NCT_TRY(hc.ready());
    NCT_TRY(apply_enqueue(ctx, model, ds, h, w, dp, p, dm, stages));
    return hc.finish();
}

int nct_region_model_apply_dev(nct_ctx* ctx, const nct_region_model* model, const uint8_t* d_src_bgr, int h, int w, const uint8_t* d_prior, const nct_region_refind_params* params,
                               uint8_t* d_mask_out) {
    NCT_CTX_ENTER();
    nct_region_refind_params p;
    NCT_TRY(apply_check(ctx, "region_model_apply_dev", model, d_src_bgr, h, w, params, d_mask_out, &p));
    const size_t N = (size_t)h * w;
    NCT_REQUIRE(!overlaps(d_mask_out, N, d_src_bgr, N * 3), "region_model_apply_dev: mask_out must not overlap src_bgr");
    NCT_REQUIRE(!d_prior || !overlaps(d_mask_out, N, d_prior, N), "region_model_apply_dev: mask_out must not overlap prior");
    return apply_enqueue(ctx, model, d_src_bgr, h, w, d_prior, p, d_mask_out, nullptr);
}

// nct_region_model_apply without a prior on the uploaded source, then nct_pair_set_region with the matte where it is: nothing goes up but the model's rows, nothing comes down
int nct_pair_apply_region_model(nct_ctx* ctx, const nct_region_model* model, const nct_region_refind_params* params, const nct_region_params* region) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (P && P->seq) return ctx->fail(NCT_ERR_STATE, "pair_apply_region_model: a sequence is open on this context (nct_seq_end closes it)");
    if (!P || !P->src || P->sh < 1) return ctx->fail(NCT_ERR_STATE, "pair_apply_region_model: no source uploaded (nct_pair_upload or nct_multi_upload first)");
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "pair_apply_region_model: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    DevBuf<uint8_t> dm;
    if (!dm.alloc(ctx, (size_t)P->sh * P->sw)) return NCT_ERR_HIP;
    nct_region_refind_params p;
    NCT_TRY(apply_check(ctx, "pair_apply_region_model", model, P->src, P->sh, P->sw, params, (uint8_t*)dm, &p));
    NCT_TRY(apply_enqueue(ctx, model, P->src, P->sh, P->sw, nullptr, p, dm, nullptr));
    return pair_set_region_dev(ctx, dm, region);             // waits for the copy: dm may go back
}

// SPEC §6.17 rules S1-S6: from the next full frame on the open sequence re-finds the model's object; NULL removes the model
int nct_seq_set_region_model(nct_ctx* ctx, const nct_region_model* model, const nct_region_refind_params* params, const nct_region_params* region) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_set_region_model");
    seq_state* q = P->seq;
    if (!model) {
        if (q->model_rows) { NCT_SYNC(); q->model_rows.reset(); }
        return NCT_OK;
    }
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "seq_set_region_model: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    nct_region_refind_params p;
    NCT_TRY(refind_params_check(ctx, "seq_set_region_model", params, &p));
    // the rows go up once, into a block the sequence keeps; the wait also covers the last frame's use of the rows they replace
    DevBuf<int16_t> rows;
    if (!rows.alloc(ctx, model->in.size() + model->out.size())) return NCT_ERR_HIP;
    NCT_H2D(rows, model->in.data(), sizeof(int16_t) * model->in.size());
    if (!model->out.empty()) NCT_H2D((int16_t*)rows + model->in.size(), model->out.data(), sizeof(int16_t) * model->out.size());
    NCT_SYNC();
    q->model_rows.take(rows);
    q->model_tap = model->tap; q->model_C = model->C; q->model_n_in = (int)(model->in.size() / model->C); q->model_n_out = (int)(model->out.size() / model->C);
    q->model_p = p; q->model_protect = region ? region->protect : 0;
    P->finished = false;                                         // what the last frame left is no longer the result of these settings
    return NCT_OK;
}

}  // extern "C"
