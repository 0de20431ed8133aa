// nct_region_select.cpp — region selection from strokes (SPEC §6.16): the chain VGG19 forward to the tap -> quantise -> seed cells -> score -> nct_resize_u8c1 -> stamp
// and snap passes on device pointers, its host and device entry points, the two seams (nct_feat_quantize, nct_region_score) and the two compositions with the region
// setters of a pair and of a sequence. Kernels: k_region_select.hip. Every transient is an arena block that goes back in stream order; nothing outlives a call.
#include "nct_pipeline.h"
#include <algorithm>

void nct_region_select_params_default(nct_region_select_params* p) {
    if (!p) return;
    p->tap = 2; p->sharpness = 1024; p->floor_permille = 700; p->max_seeds = 4096; p->snap_iters = 1;
    nct_region_snap_params_default(&p->snap);
}

// the arguments of nct_region_select[_dev] and of what is built on it (`who` names the entry point in the message); on success *p holds the parameters in force
int select_check(nct_ctx* ctx, const char* who, const void* src_bgr, int h, int w, const void* strokes, const nct_region_select_params* params, const void* mask_out,
                 nct_region_select_params* p) {
    NCT_REQUIRE(src_bgr, "%s: null src_bgr", who);
    NCT_REQUIRE(strokes, "%s: null strokes", who);
    NCT_REQUIRE(mask_out, "%s: null mask_out", who);
    NCT_REQUIRE(h >= 17 && h <= 4000, "%s: h must be in [17, 4000] (got %d)", who, h);
    NCT_REQUIRE(w >= 17 && w <= 4000, "%s: w must be in [17, 4000] (got %d)", who, w);
    if (params) *p = *params; else nct_region_select_params_default(p);
    NCT_REQUIRE(p->tap >= 1 && p->tap <= 5, "%s: tap must be in [1, 5] (got %d)", who, p->tap);
    NCT_REQUIRE(p->sharpness >= 1 && p->sharpness <= 65536, "%s: sharpness must be in [1, 65536] (got %d)", who, p->sharpness);
    NCT_REQUIRE(p->floor_permille >= 0 && p->floor_permille <= 1000, "%s: floor_permille must be in [0, 1000] (got %d)", who, p->floor_permille);
    NCT_REQUIRE(p->max_seeds >= 1 && p->max_seeds <= 4096, "%s: max_seeds must be in [1, 4096] (got %d)", who, p->max_seeds);
    NCT_REQUIRE(p->snap_iters >= 0 && p->snap_iters <= 8, "%s: snap_iters must be in [0, 8] (got %d)", who, p->snap_iters);
    NCT_TRY(nct_region_snap_params_check(ctx, who, &p->snap));
    if (nct_vgg19_weights_info(ctx, nullptr, nullptr, nullptr) != NCT_OK)
        return ctx->fail(NCT_ERR_STATE, "%s: VGG19 weights not loaded (nct_vgg19_load_caffemodel / _load_raw)", who);
    return NCT_OK;
}

// SPEC §6.16 rules 1-3 on device pointers, checked arguments: the quantised rows of the tap into r.q, the cell codes into r.code and the kept seeds' rows (inside first)
// into r.seeds. st (nullable): HOST arrays for the stages, each copied and waited for as it is made. The one wait of the plain chain is for the seed counts: the refusal
// and the launch shapes need them. with_m: rule 4's block is requested in its place between the codes and the seeds' cells
int select_seed_rows(nct_ctx* ctx, const char* who, const uint8_t* d_src, int h, int w, const uint8_t* d_strokes, const nct_region_select_params& p,
                     const nct_region_select_stages* st, bool with_m, select_rows& r) {
    hipStream_t s = ctx->stream;
    const int tap = p.tap, C = kTapC[tap - 1], ht = ((h - 1) >> (tap - 1)) + 1, wt = ((w - 1) >> (tap - 1)) + 1, cells = ht * wt;
    if (!r.q.alloc(ctx, (size_t)cells * C)) return NCT_ERR_HIP;
    NCT_TRY(select_quantised_tap(ctx, s, d_src, h, w, tap, r.q));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->q, r.q, (size_t)cells * C));
    // rule 3
    if (!r.flags.alloc(ctx, cells) || !r.pre.alloc(ctx, (size_t)cells + 1)) return NCT_ERR_HIP;
    NCT_TRY(nctk_sel_cells(ctx, s, d_strokes, h, w, tap, r.flags, r.pre));
    unsigned long long totals = 0;
    NCT_HIP(hipMemcpyAsync(&totals, (unsigned long long*)r.pre + cells, sizeof totals, hipMemcpyDeviceToHost, s));
    NCT_HIP(hipStreamSynchronize(s));
    const unsigned n_in = (unsigned)(totals & 0xffffffffull), n_out = (unsigned)(totals >> 32);
    if (n_in == 0)
        return ctx->fail(NCT_ERR_INVALID, "%s: no inside seed cell (an inside stroke must cover a cell of the tap grid that holds no outside stroke)", who);
    r.k_in = std::min(n_in, (unsigned)p.max_seeds); r.k_out = std::min(n_out, (unsigned)p.max_seeds);
    if (!r.code.alloc(ctx, cells) || (with_m && !r.m.alloc(ctx, cells)) || !r.idx.alloc(ctx, r.k_in + r.k_out) || !r.seeds.alloc(ctx, (size_t)(r.k_in + r.k_out) * C))
        return NCT_ERR_HIP;
    NCT_TRY(nctk_sel_seeds(ctx, s, r.q, r.flags, r.pre, cells, C, n_in, n_out, r.k_in, r.k_out, r.code, r.idx, r.seeds));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->cell, r.code, (size_t)cells));
    return NCT_OK;
}

// rules 1 and 2: the forward stops at the tap, whose own epilogue writes it channel-last; N1 is fused into the quantise pass. q: [cells][C], the caller's
int select_quantised_tap(nct_ctx* ctx, hipStream_t s, const uint8_t* d_src, int h, int w, int tap, int16_t* q) {
    const int C = kTapC[tap - 1], cells = (((h - 1) >> (tap - 1)) + 1) * (((w - 1) >> (tap - 1)) + 1);
    DevBuf<float> feat;
    if (!feat.alloc(ctx, (size_t)cells * C)) return NCT_ERR_HIP;
    float* taps[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    taps[tap - 1] = feat;
    NCT_TRY(nctk_vgg19_forward(ctx, s, d_src, h, w, 3 * w, tap, nullptr, nullptr, taps));
    return nctk_feat_quantize(ctx, s, feat, q, C, cells);
}

// SPEC §6.16 rules 1-6 on device pointers, checked arguments
static int select_enqueue(nct_ctx* ctx, const char* who, const uint8_t* d_src, int h, int w, const uint8_t* d_strokes, const nct_region_select_params& p, uint8_t* d_out,
                          const nct_region_select_stages* st) {
    hipStream_t s = ctx->stream;
    const int tap = p.tap, C = kTapC[tap - 1], ht = ((h - 1) >> (tap - 1)) + 1, wt = ((w - 1) >> (tap - 1)) + 1, cells = ht * wt;
    const size_t N = (size_t)h * w;
    select_rows r;
    NCT_TRY(select_seed_rows(ctx, who, d_src, h, w, d_strokes, p, st, true, r));
    const unsigned k_in = r.k_in, k_out = r.k_out;
    int16_t* const q = r.q; int16_t* const seeds = r.seeds; uint8_t* const code = r.code; uint8_t* const m = r.m;
    // rule 4
    NCT_TRY(nctk_region_score(ctx, s, q, cells, C, seeds, (int)k_in, seeds + (size_t)k_in * C, (int)k_out, p.sharpness, p.floor_permille, code, m));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->score, m, (size_t)cells));
    // rules 5 and 6: every snap pass runs out of place between d_out and one block of scratch; the first matte goes where the last pass ends in d_out
    DevBuf<uint8_t> alt, lab;
    if (p.snap_iters > 0) {
        if (!alt.alloc(ctx, N) || !lab.alloc(ctx, N * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, d_src, lab, N));
    }
    uint8_t *cur = (p.snap_iters & 1) ? (uint8_t*)alt : d_out, *oth = (p.snap_iters & 1) ? d_out : (uint8_t*)alt;
    NCT_TRY(nctk_resize_u8c1(ctx, s, m, ht, wt, cur, h, w));
    if (st) NCT_TRY(dbg_copy(ctx, s, st->up, cur, N));
    NCT_TRY(nctk_sel_stamp(ctx, s, d_strokes, N, cur));
    for (int it = 0; it < p.snap_iters; ++it) {
        NCT_TRY(nctk_region_snap(ctx, s, cur, lab, h, w, &p.snap, oth));
        std::swap(cur, oth);
        NCT_TRY(nctk_sel_stamp(ctx, s, d_strokes, N, cur));
    }
    return NCT_OK;
}

int nct_feat_quantize_check(nct_ctx* ctx, const char* who, const void* src, const char* src_name, const void* dst, const char* dst_name, int C, int H, int W) {
    NCT_REQUIRE(src, "%s: null %s", who, src_name);
    NCT_REQUIRE(dst, "%s: null %s", who, dst_name);
    NCT_REQUIRE(C > 0 && (C & 3) == 0 && C <= 4096, "%s: C must be a positive multiple of 4, at most 4096 (got %d)", who, C);
    NCT_REQUIRE(H >= 1 && W >= 1 && H <= 4096 && W <= 4096, "%s: grid %dx%d out of range", who, W, H);
    return NCT_OK;
}

extern "C" {

int nct_region_select_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, int h, int w, const uint8_t* d_strokes, const nct_region_select_params* params, uint8_t* d_mask_out) {
    NCT_CTX_ENTER();
    nct_region_select_params p;
    NCT_TRY(select_check(ctx, "region_select_dev", d_src_bgr, h, w, d_strokes, params, d_mask_out, &p));
    return select_enqueue(ctx, "region_select_dev", d_src_bgr, h, w, d_strokes, p, d_mask_out, nullptr);
}

int nct_region_select(nct_ctx* ctx, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params, uint8_t* mask_out,
                      const nct_region_select_stages* stages) {
    NCT_CTX_ENTER();
    nct_region_select_params p;
    NCT_TRY(select_check(ctx, "region_select", src_bgr, h, w, strokes, params, mask_out, &p));
    const size_t N = (size_t)h * w;
    HostCall hc(ctx);
    const uint8_t *ds = hc.in(src_bgr, N * 3), *dt = hc.in(strokes, N);
    uint8_t* dm = hc.out(mask_out, N);
    NCT_TRY(hc.ready());
    NCT_TRY(select_enqueue(ctx, "region_select", ds, h, w, dt, p, dm, stages));
    return hc.finish();
}

// rule 2 alone on a host blob in Caffe's layout: up, to channel-last, one k_feat_quantize launch, the rows down
int nct_feat_quantize(nct_ctx* ctx, const float* src_chw, int16_t* dst, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_feat_quantize_check(ctx, "feat_quantize", src_chw, "src_chw", dst, "dst", C, H, W));
    const int HW = H * W; const size_t n = (size_t)C * HW;
    HostCall hc(ctx);
    const float* t = hc.in(src_chw, n);
    float* x = hc.scratch<float>(n);
    int16_t* y = hc.out(dst, n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_chw_to_hwc(ctx, ctx->stream, t, x, C, HW));
    NCT_TRY(nctk_feat_quantize(ctx, ctx->stream, x, y, C, HW));
    return hc.finish();
}

int nct_feat_quantize_dev(nct_ctx* ctx, const float* d_src_hwc, int16_t* d_dst, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_feat_quantize_check(ctx, "feat_quantize_dev", d_src_hwc, "d_src_hwc", d_dst, "d_dst", C, H, W));
    return nctk_feat_quantize(ctx, ctx->stream, d_src_hwc, d_dst, C, H * W);
}

// rule 4 alone on host rows: the queries and the two seed lists up, one k_region_score launch, the bytes down
int nct_region_score(nct_ctx* ctx, const int16_t* q, int cells, int C, const int16_t* seeds_in, int n_in, const int16_t* seeds_out, int n_out, int sharpness, int floor_permille,
                     uint8_t* score_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_score_check(ctx, "region_score", q, cells, C, seeds_in, n_in, seeds_out, n_out, sharpness, floor_permille, score_out));
    HostCall hc(ctx);
    const int16_t *dq = hc.in(q, (size_t)cells * C), *di = hc.in(seeds_in, (size_t)n_in * C);
    const int16_t* dn = n_out > 0 ? hc.in(seeds_out, (size_t)n_out * C) : nullptr;          // no outside rows: the launcher never reads the list
    uint8_t* dm = hc.out(score_out, cells);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_region_score(ctx, ctx->stream, dq, cells, C, di, n_in, dn, n_out, sharpness, floor_permille, nullptr, dm));
    return hc.finish();
}

int nct_region_score_dev(nct_ctx* ctx, const int16_t* d_q, int cells, int C, const int16_t* d_seeds_in, int n_in, const int16_t* d_seeds_out, int n_out, int sharpness,
                         int floor_permille, uint8_t* d_score_out) {
    NCT_CTX_ENTER();
    return nctk_region_score(ctx, ctx->stream, d_q, cells, C, d_seeds_in, n_in, d_seeds_out, n_out, sharpness, floor_permille, nullptr, d_score_out);
}

// measurement hook: the mean device time of one k_region_score launch, between two events on the library's stream
int nct_region_score_bench(nct_ctx* ctx, const int16_t* d_q, int cells, int C, const int16_t* d_seeds_in, int n_in, const int16_t* d_seeds_out, int n_out, int sharpness,
                           int floor_permille, uint8_t* d_score_out, int reps, float* kernel_ms) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(kernel_ms, "region_score_bench: null kernel_ms");
    NCT_REQUIRE(reps >= 1 && reps <= 1000, "region_score_bench: reps must be in [1, 1000] (got %d)", reps);
    NCT_TRY(nctk_region_score(ctx, ctx->stream, d_q, cells, C, d_seeds_in, n_in, d_seeds_out, n_out, sharpness, floor_permille, nullptr, d_score_out));   // warm-up
    NCT_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < reps; ++r)
        NCT_TRY(nctk_region_score(ctx, ctx->stream, d_q, cells, C, d_seeds_in, n_in, d_seeds_out, n_out, sharpness, floor_permille, nullptr, d_score_out));
    NCT_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    NCT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    NCT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *kernel_ms = ms / reps;
    return NCT_OK;
}

// nct_region_select on the uploaded source, then nct_pair_set_region with the matte where it is: the strokes go up, nothing comes down
int nct_pair_select_region(nct_ctx* ctx, const uint8_t* strokes, const nct_region_select_params* params, const nct_region_params* region) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (P && P->seq) return ctx->fail(NCT_ERR_STATE, "pair_select_region: a sequence is open on this context (nct_seq_end closes it)");
    if (!P || !P->src || P->sh < 1) return ctx->fail(NCT_ERR_STATE, "pair_select_region: no source uploaded (nct_pair_upload or nct_multi_upload first)");
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "pair_select_region: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    const size_t N = (size_t)P->sh * P->sw;
    DevBuf<uint8_t> dt, dm;
    if (!dt.alloc(ctx, N) || !dm.alloc(ctx, N)) return NCT_ERR_HIP;
    nct_region_select_params p;
    NCT_TRY(select_check(ctx, "pair_select_region", P->src, P->sh, P->sw, strokes, params, (uint8_t*)dm, &p));
    NCT_H2D(dt, strokes, N);
    NCT_TRY(select_enqueue(ctx, "pair_select_region", P->src, P->sh, P->sw, dt, p, dm, nullptr));
    return pair_set_region_dev(ctx, dm, region);             // waits for the copy: dm may go back
}

// nct_region_select on a frame of the open sequence's size, then nct_seq_set_region with the matte where it is
int nct_seq_select_region(nct_ctx* ctx, const uint8_t* frame_bgr, const uint8_t* strokes, const nct_region_select_params* params, const nct_region_params* region) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_select_region");
    if (P->seq->target())
        return ctx->fail(NCT_ERR_STATE, "seq_select_region: not defined in a full-resolution sequence (select on the frame with nct_region_select, then nct_seq_set_region)");
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "seq_select_region: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    NCT_REQUIRE(frame_bgr, "seq_select_region: null frame_bgr");
    const size_t N = (size_t)P->sh * P->sw;
    DevBuf<uint8_t> ds, dt, dm;
    if (!ds.alloc(ctx, N * 3) || !dt.alloc(ctx, N) || !dm.alloc(ctx, N)) return NCT_ERR_HIP;
    nct_region_select_params p;
    NCT_TRY(select_check(ctx, "seq_select_region", frame_bgr, P->sh, P->sw, strokes, params, (uint8_t*)dm, &p));
    NCT_H2D(ds, frame_bgr, N * 3); NCT_H2D(dt, strokes, N);
    NCT_TRY(select_enqueue(ctx, "seq_select_region", ds, P->sh, P->sw, dt, p, dm, nullptr));
    return seq_set_region_dev(ctx, dm, region);
}

}  // extern "C"
