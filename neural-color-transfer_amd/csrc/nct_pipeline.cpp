// nct_pipeline.cpp — the per-pair hot loop: the MI355X counterpart of transfer_color_single_bds (main.cu:47-454).
// Everything between "two BGR images in" and "one BGR image out" stays on the device: no per-level cudaMalloc/Free churn
// (main.cu:238-257,297-326), no D2H of NNFs/error maps (main.cu:286-289,318), no host-side BDS vote (main.cu:291),
// no CSR ping-pong for the solvers. S features are recomputed from the intermediate result only up to the tap the
// next level needs (1115 instead of 2297 GFLOP per 700x700 pair, identical values).
// Here: the pair / multi-reference run (pair_run), finish_level, the full-resolution pair, nct_pair_fit_lut. Sequences: nct_seq.cpp; what both share: nct_pipeline.h.
#include "nct_pipeline.h"
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <cmath>

pair_state* pair_of(nct_ctx* ctx) {
    if (!ctx->pair) ctx->pair = new pair_state();
    return (pair_state*)ctx->pair;
}
void drop_images(pair_state* P) {
    P->src.reset(); P->out.reset(); P->full_src.reset(); P->full_out.reset(); P->mask.reset(); P->full_mask.reset(); P->fin_mask.reset();
    for (DevBuf<uint8_t>& r : P->ref) r.reset();
    for (DevBuf<uint8_t>& m : P->rmask) m.reset();
    P->K = 0; P->finished = false; P->protect = 0;
}
// the images live in the context arena like every other device buffer (no hipMalloc/hipFree — device-wide synchronisation points —
// between the pairs of other contexts in flight on the same GPU). The sequence's and the images' owners give their blocks back here: the arena still holds them
void nct_pair_free(nct_ctx* ctx) {
    if (!ctx->pair) return;
    seq_free((pair_state*)ctx->pair);
    delete (pair_state*)ctx->pair; ctx->pair = nullptr;
}

static int read_marks(nct_ctx* ctx, nct_pair_timing* t) {
    double* acc[9] = {&t->other_ms, &t->vgg_ms, &t->cluster_ms, &t->patchmatch_ms, &t->vote_ms, &t->knn_ms, &t->color_ms, &t->nonlocal_ms, &t->wls_ms};
    for (size_t i = 1; i < ctx->tm_tags.size(); ++i) {
        float ms = 0.f;
        NCT_HIP(hipEventElapsedTime(&ms, ctx->tm_events[i - 1], ctx->tm_events[i]));
        const int stage = ctx->tm_tags[i] >> 3, level = ctx->tm_tags[i] & 7;
        if (stage >= 0 && stage < 9) *acc[stage] += ms;
        if (level < 5) {
            if (stage == NCT_ST_PM) t->pm_level_ms[level] += ms;
            else if (stage == NCT_ST_VOTE) t->vote_level_ms[level] += ms;
            else if (stage == NCT_ST_NONLOCAL) t->nonlocal_level_ms[level] += ms;
            else if (stage == NCT_ST_WLS) t->wls_level_ms[level] += ms;
        }
    }
    if (getenv("NCT_HOST_TRACE") && ctx->tm_host.size() == ctx->tm_tags.size()) {
        static const char* names[9] = {"other", "vgg", "cluster", "pm", "vote", "knn", "color", "nonlocal", "wls"};
        for (size_t i = 1; i < ctx->tm_tags.size(); ++i) {
            float ms = 0.f; (void)hipEventElapsedTime(&ms, ctx->tm_events[0], ctx->tm_events[i]);
            fprintf(stderr, "nct mark %-8s L%d  host %8.3f ms  gpu %8.3f ms\n", names[(ctx->tm_tags[i] >> 3) % 9], ctx->tm_tags[i] & 7, (ctx->tm_host[i] - ctx->tm_host[0]) / 1000.0, ms);
        }
    }
    t->color_ms += t->nonlocal_ms + t->wls_ms;       // color_ms is the whole stage; the two solves are also reported on their own
    return 0;
}

run_clock::run_clock(nct_ctx* c, nct_pair_timing* t, int flags) : ctx(c), timing(t), wall0(std::chrono::steady_clock::now()) {
    if (timing) memset(timing, 0, sizeof *timing);
    ctx->tm_on = timing != nullptr; ctx->tm_tags.clear(); ctx->tm_host.clear();
    ctx->kt_on = timing != nullptr && (flags & NCT_FLAG_TIME_KERNELS) != 0; ctx->kt_ids.clear();
    ctx->wls_split = (flags & NCT_FLAG_LATENCY) ? 1 : 0;
}
// what a finished run (the main stream has been synchronised) leaves for nct_pair_timing: total_ms, the stage marks, the kernel clock, the evaluation counters
int run_clock::read(bool count) {
    if (!timing) return NCT_OK;
    timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    NCT_TRY(read_marks(ctx, timing));
    for (size_t i = 0; i < ctx->kt_ids.size(); ++i) {               // NCT_FLAG_TIME_KERNELS: average the samples per kernel
        float ms = 0.f;
        NCT_HIP(hipEventElapsedTime(&ms, ctx->kt_events[2 * i], ctx->kt_events[2 * i + 1]));
        const int id = ctx->kt_ids[i];
        if (id >= 0 && id < 10) { timing->kernel_us[id] += 1e3 * ms; timing->kernel_samples[id] += 1; }
    }
    for (int id = 0; id < 10; ++id) if (timing->kernel_samples[id]) timing->kernel_us[id] /= timing->kernel_samples[id];
    if (count) {
        unsigned long long h[32];
        NCT_HIP(hipMemcpy(h, ctx->d_counter, sizeof h, hipMemcpyDeviceToHost));
        for (int l = 0; l < 5; ++l) { timing->pm_level_evals[l] = h[4 * l]; timing->pm_level_accepted[l] = h[4 * l + 1]; }
    }
    return 0;
}


int full_lab::open(nct_ctx* ctx, hipStream_t s, const full_target* full) {
    if (!full || full->finish != NCT_FINISH_EXACT) return NCT_OK;
    const size_t N0 = (size_t)full->H * full->W;
    if (!s0.alloc(ctx, N0 * 3) || !out0.alloc(ctx, N0 * 3)) return NCT_ERR_HIP;
    return nctk_bgr2lab(ctx, s, full->src, s0, N0);
}
int finish_level(nct_ctx* ctx, hipStream_t s, const double* x, int h, int w, int H, int W, const uint8_t* s_lab_full, uint8_t* out_lab, uint8_t* out_bgr,
                 const full_target* full, const full_lab& fl, const nct_color_params& cp, const nct_color_debug* dbg, int cube, const region_fin* region) {
    if (full && full->finish == NCT_FINISH_EXACT) {
        NCT_TRY(nctk_color_finish(ctx, s, x, h, w, H, W, fl.s0, full->H, full->W, cp, fl.out0, dbg));
        if (region) return nctk_region_compose(ctx, s, full->src, fl.s0, fl.out0, region->mask, (size_t)full->H * full->W, region->protect, cube, full->out);
        return nctk_lab2bgr(ctx, s, fl.out0, full->out, (size_t)full->H * full->W, cube);
    }
    const nct_finish_up up{full ? full->src : nullptr, full ? full->H : 0, full ? full->W : 0, full ? full->out : nullptr, cube, ctx->guided_sigma /* nct_set_finish_guided */,
                           full && region ? full->mask : nullptr, region ? region->protect : 0};
    NCT_TRY(nctk_color_finish(ctx, s, x, h, w, H, W, s_lab_full, H, W, cp, out_lab, dbg, full ? &up : nullptr));
    if (region) return nctk_region_compose(ctx, s, region->s_bgr, s_lab_full, out_lab, region->mask, (size_t)H * W, region->protect, cube, out_bgr);
    return nctk_lab2bgr(ctx, s, out_lab, out_bgr, (size_t)H * W, cube);
}
int finish_level_masked(nct_ctx* ctx, hipStream_t s, masked_fin& mf, const double* x_from, DevBuf<double>& x_mix, DevBuf<uint8_t>& m_buf, DevBuf<uint8_t>& f_buf,
                        DevBuf<uint8_t>& fin_mask, int h, int w, int H, int W, const uint8_t* s_lab_full, uint8_t* out_lab, uint8_t* out_bgr, const full_target* full,
                        const full_lab& fl, const nct_color_params& cp, const nct_color_debug* dbg, int cube) {
    const size_t n = (size_t)h * w;
    const bool exact = full && full->finish == NCT_FINISH_EXACT;          // the upsampling finish composes at the working size (and, in its own pass, on the original)
    const bool up = mf.p_l && full && !exact;                             // the masked upsampling finish with a reference mask (SPEC §6.19 rule 8)
    mf.fh = exact ? full->H : H; mf.fw = exact ? full->W : W;
    mf.f_l = exact ? full->mask : mf.mask_work;
    full_target up_target;
    const bool make_m = !mf.m_l;
    if (make_m) mf.m_l = mf.p_l ? mf.p_l : mf.mask_l;
    if (mf.p_l) {
        if (make_m && mf.mask_l) {
            // SPEC §6.12 rule 4 on one map: M_l = min(P_l, the source's level mask)
            if (!m_buf.reserve(ctx, n)) return NCT_ERR_HIP;
            NCT_TRY(nctk_region_merge(ctx, s, &mf.p_l, 1, nullptr, mf.mask_l, (int)n, nullptr, m_buf));
            mf.m_l = m_buf;
        }
        // rule 5: F_l = P_l at the size the finish targets, then the minimum with the source's mask there. The last level's has the size of the result and is kept
        // (rule 7) — unless the masked upsampling finish keeps F0 there: then F_l is scratch like every other level's
        const bool keep_f = mf.last && !up;
        DevBuf<uint8_t>& f = keep_f ? fin_mask : f_buf;
        if (keep_f ? !f.alloc(ctx, (size_t)mf.fh * mf.fw) : !f.reserve(ctx, (size_t)H * W)) return NCT_ERR_HIP;
        NCT_TRY(nctk_region_upsize_min(ctx, s, mf.p_l, h, w, mf.f_l, f, mf.fh, mf.fw));
        mf.f_l = f;
        if (up) {
            // the upsampling pass composes on the original with F0 = min(resize(P' -> H0 x W0), M0); it has the result's size and is kept as fin_mask
            if (!fin_mask.alloc(ctx, (size_t)full->H * full->W)) return NCT_ERR_HIP;
            NCT_TRY(nctk_region_upsize_min(ctx, s, mf.p_l, h, w, full->mask, fin_mask, full->H, full->W));
            up_target = *full; up_target.mask = fin_mask; full = &up_target;
        }
    }
    // SPEC §6.11 rule 2: the coefficients move toward the identity by M_l — in place (a run that is no frame of a sequence), or out of place from the kept X'
    if (!x_mix.reserve(ctx, 6 * n)) return NCT_ERR_HIP;
    NCT_TRY(nctk_region_mix(ctx, s, x_from, mf.m_l, h, w, x_mix));
    const region_fin rg{mf.f_l, mf.s_bgr, mf.protect};
    return finish_level(ctx, s, x_mix, h, w, H, W, s_lab_full, out_lab, out_bgr, full, fl, cp, dbg, cube, &rg);
}

// what one reference owns during a run (SPEC §6.2): its image pyramid, its five un-normalised taps (HWC, indexed by level), its NNFs of both directions (kept from
// level to level) and its R -> S distances; with several references also its G_k and E_k
struct ref_bufs {
    int bh[5], bw[5], rs_range[5];
    DevBuf<uint8_t> pyr[5];
    DevBuf<float> feat[5];
    DevBuf<uint32_t> ann, bnn, ann_prev, bnn_prev;
    DevBuf<float> bnnd, err;
    DevBuf<uint8_t> guide;
    const uint8_t* img[5];
    // the reference's region mask (SPEC §6.12; qimg[4] null: none): its level masks Q_k,l beside the image pyramid, and P_k,l, the current level's mask pulled to S's grid
    DevBuf<uint8_t> qpyr[4], pulled; const uint8_t* qimg[5] = {};
    const float* featp[5];                          // the taps the correspondence reads: feat[l], or the ones an open sequence prepared (SPEC §6.3)
};

// What the side stream writes: per level that runs, S's level image in Lab, its kNN graph and the graph-only part of S1's system (reverse adjacency, hub block
// table: k_s1.hip), built behind each graph. THE RULE: no arena block that the side stream may still read or write is marked free before stream2 has been
// synchronised. So the destructor first waits for the side stream, ends the deferral and frees what was released meanwhile, and only then do the members go back —
// on every way out of a run, the error returns included. What the side stream only reads (S's pyramid, the labels) belongs to members of pair_run declared
// in front of this one, which are therefore released after it.
struct side_bufs {
    nct_ctx* ctx;
    DevBuf<uint8_t> slab[5];
    DevBuf<int> knn_ids[5];
    DevBuf<double> knn_ws[5];
    nct_s1_graph_bufs s1g[5];
    explicit side_bufs(nct_ctx* c) : ctx(c) {}
    ~side_bufs() { (void)hipStreamSynchronize(ctx->stream2); ctx->defer_release = false; ctx->flush_deferred(); }
};

static const nct_multi_levels kNoLevels = {};

// One run of the L=5->1 loop on the device-resident source and its K references: the state its stages share and, as members in the order the stages allocate them,
// every buffer of the run (the arena is best-fit over cached blocks: order and sizes decide what a context holds afterwards). With K = 1 this enqueues a pair's
// launches and nothing else.
struct pair_run {
    nct_ctx* const ctx; const nct_params* const prm; nct_pair_timing* const timing;
    const nct_multi_levels* const lv;              // where the level intermediates go (every pointer nullable): a pair reports as the list of one reference
    const nct_color_stages* const* const color;    // nullable: [5] the colour stage's coefficient maps a pair may ask for
    const full_target* const fin;                  // nullable: the last level finishes on the original source (finish_level)
    seq_state* const seq;                          // nullable: this run is a frame of the open sequence (SPEC §6.3) — the reference's pyramid and taps are borrowed, S1's output is blended
    const nct_seq_levels* const slv;               // nullable: where a frame's X'_t and tau_p maps go
    const nct_ref_region_levels* const qlv;        // nullable: where a masked run's level masks and mixed coefficients go (SPEC §6.11, §6.12)
    const nct_seq_hold_levels* const hlv;          // nullable: where a frame over several references reports the held selection's free labels and margins (SPEC §6.18)
    const nct_seq_pull_levels* const plv;          // nullable: where a frame with a reference mask reports the merged pull before and after its hold (SPEC §6.19)
    pair_state* const P; const hipStream_t s;
    const int H, W, K, nlevels; const size_t N;
    const bool feat16, count;
    size_t NR = 0;                                 // pixels of the largest reference: the shared scratch of R's normalised features
    int ah[5], aw[5];
    const uint8_t* simg[5];
    ref_bufs R[NCT_MAX_REFS];
    DevBuf<uint8_t> s_lab_full, spyr[5];
    DevBuf<float> sfeat;                           // S features of the current level, channel-last (largest: H x W x 64)
    DevBuf<int> labels, nlab_dev;
    DevBuf<float> na, nb, voted, nvoted;
    DevBuf<uint16_t> na_h, nb_h;                   // fp16 shadow maps of the normalised features: the candidate tiles of the opt-in reduced-precision mode (NCT_FLAG_FEAT16)
    side_bufs side;
    // annd is scratch shared by the references. err / guide: what the colour stage reads — reference 0's own maps with K = 1, the merged maps (rule 3) with several
    DevBuf<float> annd, err;
    DevBuf<uint8_t> guide, g_lab_l, out_lab;
    DevBuf<uint8_t> sel_label;                     // the selection's label map (rule 2); a pair allocates none of this
    // SPEC §6.18: this frame of a sequence over several references selects with a memory — it has a previous frame to hold against, it blends and hold > 0. Every other
    // frame runs rule 2 as it stands; both keep their label map in the sequence. field_found: the level's field was found in front of the selection, the blend reads it
    const bool held;
    bool field_found = false;
    // SPEC §6.23: carry_keep — this frame of a carrying sequence keeps every level's final fields; carry_merge — it also has kept fields to move and merge
    const bool carry_keep, carry_merge;
    // The run's masks (neither: the run enqueues and reserves what it always did). mask: the source's region mask (SPEC §6.11; null: none), mpyr / mimg: its level masks —
    // the pyramid's single-channel form. ref_masked: a reference has a region mask (SPEC §6.12); p_merged: P_l of several references (rule 3), m_level: M_l where it is not
    // P_l itself (rule 4: a source mask as well), f_level: F_l of a level that is not the last (the last level's is pair_state's fin_mask).
    // What a level's colour stage reads of all that (level_masks, color_stage): p_l and m_l, the mix mask on the level grid; the compose mask is finish_level_masked's
    const uint8_t* mask;                           // a tracked frame of a sequence (SPEC §6.14) carries the matte first: lab_and_pyramids reads the pointer again
    DevBuf<uint8_t> mpyr[4]; const uint8_t* mimg[5] = {};
    const bool ref_masked;
    // SPEC §6.19: this frame of a sequence with a reference mask holds its merged pull against the map the previous frame kept — it blends and such a map exists. Every
    // other masked frame keeps P_l as it is. hold_lab: L_t[l] for the hold (and the held selection, which then makes it), given back behind the hold. up_masked: the
    // last level finishes through the masked upsampling finish with F0, made from P' at the original size
    const bool pull_hold, up_masked;
    DevBuf<uint8_t> hold_lab;
    // SPEC §6.17: this full frame of a sequence with a region model re-finds its matte behind the forward (not the own frame of a fresh matte: rule S1). tapfeat: the
    // model's tap of that forward, channel-last, where it is not conv5_1 itself. The level masks are then built behind the re-find: nothing reads them before level 0's mix
    const bool refind;
    DevBuf<float> tapfeat;
    DevBuf<uint8_t> p_merged, m_level, f_level;
    const uint8_t *p_l = nullptr, *m_l = nullptr;
    const nct_color_params cp;

    pair_run(nct_ctx* c, const nct_params* p, nct_pair_timing* t, const run_extras& x)
        : ctx(c), prm(p), timing(t), lv(x.lv ? x.lv : &kNoLevels), color(x.color), fin(x.fin), seq(x.seq), slv(x.slv), qlv(x.qlv), hlv(x.hlv), plv(x.plv), P((pair_state*)c->pair), s(c->stream), H(P->sh), W(P->sw), K(P->K),
          nlevels(p->levels), N((size_t)H * W), feat16((p->flags & NCT_FLAG_FEAT16) != 0), count(t && (p->flags & NCT_FLAG_COUNT_EVALS)), side(c), held(x.seq && P->K > 1 && x.seq->frames > 0 && x.seq->tau > 0.0 && x.seq->hold > 0.0),
          carry_keep(x.seq && x.seq->carry), carry_merge(x.seq && x.seq->carry && x.seq->carry_kept && x.seq->frames > 0), mask(P->mask),
          ref_masked(P->ref_masked()), pull_hold(ref_masked && x.seq && x.seq->frames > 0 && x.seq->tau > 0.0 && x.seq->pull_kept),
          up_masked(ref_masked && x.fin && x.fin->finish == NCT_FINISH_UPSAMPLE), refind(x.seq && x.seq->model_rows && !(P->mask && x.seq->matte_fresh)), cp(nct_color_params_of(*p)) {}

    int d2h(void* dst, const void* src, size_t bytes) {
        if (dst) NCT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        return 0;
    }

    // level geometry, coarse -> fine (level 0 = conv5_1)
    void geometry() {
        level_sizes(H, W, ah, aw);
        for (int k = 0; k < K; ++k) {
            level_sizes(P->rh[k], P->rw[k], R[k].bh, R[k].bw);
            // the random-search radius of reference k is the pair (S, R_k)'s own (SPEC §6.2 rule 1), not the largest reference's
            const int maxLen = std::max(std::max(W, H), std::max(P->rw[k], P->rh[k]));
            const int rs[5] = {maxLen / 16, maxLen / 32, maxLen / 64, 32, 32};                     // main.cu:77-83
            for (int l = 0; l < 5; ++l) R[k].rs_range[l] = rs[l];
            NR = std::max(NR, (size_t)P->rh[k] * P->rw[k]);
        }
    }

    // SPEC §6.11 rule 1: the level masks, each resized from the level above like the image pyramid
    int source_level_masks() {
        mimg[4] = mask;
        return source_mask_levels(ctx, s, mpyr, mimg, ah, aw, 0);
    }

    // SPEC §6.17 rules S2-S5: the frame's matte from the tap its own forward has just written, then the level masks of that matte. Its time counts as other_ms
    int refind_masks() {
        NCT_TRY(seq_refind_step(ctx, s, P, seq, tapfeat.ok() ? (const float*)tapfeat : (const float*)sfeat, s_lab_full));
        tapfeat.reset();                                             // given back early: the level loop's requests come behind it
        mask = P->mask;
        NCT_TRY(source_level_masks());
        MARK(NCT_ST_OTHER, 0);
        return NCT_OK;
    }

    // S in Lab (ColorTransfer ctor, ColorTransfer.h:54-75) and image pyramids (main.cu:104-108)
    int lab_and_pyramids() {
        if (!s_lab_full.alloc(ctx, N * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, P->src, s_lab_full, N));
        simg[4] = P->src;
        for (int k = 0; k < K; ++k) R[k].img[4] = P->ref[k];
        for (int l = 3; l >= 0; --l) {
            NCT_TRY(pyramid_level(ctx, s, spyr[l], simg, ah, aw, l));
            if (seq) { for (int k = 0; k < K; ++k) R[k].img[l] = seq->rpyr[k][l]; continue; }          // the sequence's reference pyramids were built at nct_seq_begin
            for (int k = 0; k < K; ++k) NCT_TRY(pyramid_level(ctx, s, R[k].pyr[l], R[k].img, R[k].bh, R[k].bw, l));
        }
        // SPEC §6.14: a tracked sequence's matte follows the frame's field before its level masks are built; the two matte blocks may have changed places
        if (seq && mask) { NCT_TRY(seq_track_step(ctx, s, P, seq, simg, s_lab_full)); mask = P->mask; }
        if (mask && !refind) NCT_TRY(source_level_masks());
        for (int k = 0; k < K && ref_masked; ++k) {
            // SPEC §6.12 rule 1: the masked references' level masks, on the reference's level grids
            if (!P->rmask[k]) continue;
            R[k].qimg[4] = P->rmask[k];
            if (seq) { for (int l = 3; l >= 0; --l) R[k].qimg[l] = seq->rq[k][l]; continue; }          // the sequence's level masks were built by nct_seq_set_ref_region (SPEC §6.19)
            for (int l = 3; l >= 0; --l) {
                if (!R[k].qpyr[l].alloc(ctx, (size_t)R[k].bh[l] * R[k].bw[l])) return NCT_ERR_HIP;
                NCT_TRY(nctk_resize_u8c1(ctx, s, R[k].qimg[l + 1], R[k].bh[l + 1], R[k].bw[l + 1], R[k].qpyr[l], R[k].bh[l], R[k].bw[l]));
                R[k].qimg[l] = R[k].qpyr[l];
            }
        }
        MARK(NCT_ST_OTHER, 0);
        return NCT_OK;
    }

    // VGG19: R once (all five taps kept, HWC), S to conv5_1 (main.cu:94,102)
    int forwards() {
        if (!sfeat.alloc(ctx, (size_t)64 * N)) return NCT_ERR_HIP;
        if (seq) {
            // the reference's taps are the sequence's (one forward at nct_seq_begin): S runs to conv5_1 on its own. Every conv output is its own fmaf chain, so the
            // bytes are those of the paired launch
            for (int k = 0; k < K; ++k) for (int l = 0; l < 5; ++l) R[k].featp[l] = seq->rfeat[k][l];
            float* staps_hwc[5] = {nullptr, nullptr, nullptr, nullptr, sfeat};
            if (refind && seq->model_tap < 5) {
                // SPEC §6.17 rule S2: the forward also stores the model's tap channel-last; no second forward
                const int t = seq->model_tap - 1;
                if (!tapfeat.alloc(ctx, (size_t)kTapC[t] * ah[4 - t] * aw[4 - t])) return NCT_ERR_HIP;
                staps_hwc[t] = tapfeat;
            }
            NCT_TRY(nctk_vgg19_forward(ctx, s, P->src, H, W, W * 3, 5, nullptr, nullptr, staps_hwc));
            MARK(NCT_ST_VGG, 0);
            return NCT_OK;
        }
        for (int k = 0; k < K; ++k) {
            // the five taps of R arrive channel-last straight from their conv layers' epilogues (round 4: no CHW -> HWC transpose pass)
            float* taps_hwc[5];
            for (int t = 0; t < 5; ++t) {
                const int l = 4 - t;
                if (!R[k].feat[l].alloc(ctx, (size_t)kTapC[t] * R[k].bh[l] * R[k].bw[l])) return NCT_ERR_HIP;
                taps_hwc[t] = R[k].feat[l]; R[k].featp[l] = R[k].feat[l];
            }
            if (k == 0) {
                // R and S together: conv5_1 of both images is one launch (two grids of 124 workgroups at 700 x 700 would each leave half the chip idle)
                float* staps_hwc[5] = {nullptr, nullptr, nullptr, nullptr, sfeat};
                NCT_TRY(nctk_vgg19_forward_pair(ctx, s, P->ref[0], P->rh[0], P->rw[0], P->rw[0] * 3, taps_hwc, P->src, H, W, W * 3, staps_hwc));
            } else {
                // the further references (SPEC §6.2) have no partner for their last layer: a forward of their own
                NCT_TRY(nctk_vgg19_forward(ctx, s, P->ref[k], P->rh[k], P->rw[k], P->rw[k] * 3, 5, nullptr, nullptr, taps_hwc));
            }
        }
        MARK(NCT_ST_VGG, 0);
        return NCT_OK;
    }

    // C1: cluster the coarsest S features (main.cu:139-168)
    int cluster() {
        if (!labels.alloc(ctx, (size_t)ah[0] * aw[0]) || !nlab_dev.alloc(ctx, 1)) return NCT_ERR_HIP;
        if (!na.alloc(ctx, (size_t)64 * N) || !nb.alloc(ctx, (size_t)64 * NR) || !voted.alloc(ctx, (size_t)64 * N) || !nvoted.alloc(ctx, (size_t)64 * N)) return NCT_ERR_HIP;
        if (!na_h.alloc(ctx, feat16 ? (size_t)64 * N : 8) || !nb_h.alloc(ctx, feat16 ? (size_t)64 * NR : 8)) return NCT_ERR_HIP;
        NCT_TRY(nctk_normalize(ctx, s, sfeat, na, nullptr, 512, ah[0] * aw[0], feat16 ? (uint16_t*)na_h : nullptr));
        NCT_TRY(nctk_kmeans_labels(ctx, s, na, ah[0] * aw[0], 512, prm->cluster_num, 11, (uint64_t)prm->seed, labels, nlab_dev));
        // the number of labels (1 if k-means degenerated, else K) stays on the device: reading it back would stall the host — and with it
        // the enqueueing of everything below — until the VGG forwards and k-means have finished
        MARK(NCT_ST_CLUSTER, 0);
        return NCT_OK;
    }

    // what the level loop (main.cu:179-428) works in, and the result image
    int level_buffers() {
        for (int k = 0; k < K; ++k) {
            const size_t nr = (size_t)P->rh[k] * P->rw[k];
            if (!R[k].ann.alloc(ctx, N) || !R[k].bnn.alloc(ctx, nr) || !R[k].ann_prev.alloc(ctx, N) || !R[k].bnn_prev.alloc(ctx, nr)) return NCT_ERR_HIP;
        }
        if (!annd.alloc(ctx, N)) return NCT_ERR_HIP;
        for (int k = 0; k < K; ++k) if (!R[k].bnnd.alloc(ctx, (size_t)P->rh[k] * P->rw[k])) return NCT_ERR_HIP;
        if (!err.alloc(ctx, N) || !guide.alloc(ctx, N * 3) || !g_lab_l.alloc(ctx, N * 3) || !out_lab.alloc(ctx, N * 3)) return NCT_ERR_HIP;
        if (K > 1) {
            if (!sel_label.alloc(ctx, N)) return NCT_ERR_HIP;
            for (int k = 0; k < K; ++k) if (!R[k].err.alloc(ctx, N) || !R[k].guide.alloc(ctx, N * 3)) return NCT_ERR_HIP;
        }
        if (ref_masked) {
            for (int k = 0; k < K; ++k) if (R[k].qimg[4] && !R[k].pulled.alloc(ctx, N)) return NCT_ERR_HIP;
            if (K > 1 && (!pull_hold || plv) && !p_merged.alloc(ctx, N)) return NCT_ERR_HIP;      // a frame that holds merges inside the hold; the free P_l is kept only for the report
            if (mask && !m_level.alloc(ctx, N)) return NCT_ERR_HIP;
            if ((nlevels > 1 || up_masked) && !f_level.alloc(ctx, N)) return NCT_ERR_HIP;      // one level: its F is the last level's, pair_state's fin_mask (the masked upsampling finish keeps F0 there)
        }
        if (!P->out.reserve(ctx, N * 3)) return NCT_ERR_HIP;
        return d2h(lv->labels, labels, sizeof(int) * (size_t)ah[0] * aw[0]);
    }

    // K1 for the levels that run (nct_params.levels) on the side stream: the kNN graph of a level depends only on the level image of S and on the
    // labels (main.cu:351-359), not on the correspondence, so it overlaps with PatchMatch / votes / solvers of the main stream
    // (whose many small launches leave most CUs idle). Scratch released meanwhile stays reserved until the join (nct_internal.h).
    // Enqueued from inside the level loop, AFTER the coarsest level's correspondence work has been submitted: the side stream's ~200
    // small packets would otherwise sit in front of the main stream's and the main stream starts the level loop ~2.6 ms late
    int enqueue_side_graphs() {
        // arena blocks are recycled in stream order: the side stream may reuse blocks the main stream released up to this point, so it
        // starts behind everything enqueued on the main stream so far
        hipStream_t s2 = ctx->stream2;
        NCT_HIP(hipEventRecord(ctx->ev_fork, s));
        NCT_HIP(hipStreamWaitEvent(s2, ctx->ev_fork, 0));
        for (int l = 0; l < nlevels; ++l) {
            const size_t npx = (size_t)ah[l] * aw[l];
            if (!side.slab[l].alloc(ctx, npx * 3) || !side.knn_ids[l].alloc(ctx, npx * 8) || !side.knn_ws[l].alloc(ctx, npx * 8) || !side.s1g[l].alloc(ctx, (int)npx)) return NCT_ERR_HIP;
        }
        int rc = 0;
        ctx->defer_release = true;
        for (int l = 0; l < nlevels && rc == 0; ++l) {      // only the levels that run (nct_params.levels)
            rc = nctk_bgr2lab(ctx, s2, simg[l], side.slab[l], (size_t)ah[l] * aw[l]);
            if (rc == 0) rc = nctk_knn_graph(ctx, s2, side.slab[l], ah[l], aw[l], labels, ah[0], aw[0], 0, nlab_dev, 1 << l, side.knn_ids[l], side.knn_ws[l]);
            // S1's reverse adjacency and hub block table depend on the graph alone: built here, off the main stream; the block count lands in page-locked memory
            // before ev_level[l] completes, so the host can size (or skip) the level's hub passes without a synchronisation
            if (rc == 0) rc = nctk_s1_graph_build(ctx, s2, side.knn_ids[l], side.knn_ws[l], sqrt(prm->nonlocal_weight / (double)prm->k_num), side.s1g[l].view(-1, -1), ctx->s1_hub_blocks() + 2 * l);
            if (rc == 0 && hipEventRecord(ctx->ev_level[l], s2) != hipSuccess) rc = ctx->fail(NCT_ERR_HIP, "hipEventRecord failed");
        }
        ctx->defer_release = false;
        return rc;
    }

    // the correspondence of level l with reference k (SPEC §6.2 rule 1): NNFs, PatchMatch both directions, BDS votes, matching error
    int correspondence(int l, int k) {
        const int C = kTapC[4 - l];
        const int* bh = R[k].bh; const int* bw = R[k].bw;
        const int na_px = ah[l] * aw[l], nb_px = bh[l] * bw[l];
        uint32_t *ann = R[k].ann, *bnn = R[k].bnn, *ann_prev = R[k].ann_prev, *bnn_prev = R[k].bnn_prev;
        float* bnnd = R[k].bnnd;
        // NNF init / upsample (main.cu:230-251)
        if (l == 0) {
            NCT_TRY(nctk_nnf_init(ctx, s, ann, ah[0], aw[0], bh[0], bw[0]));
            NCT_TRY(nctk_nnf_init(ctx, s, bnn, bh[0], bw[0], ah[0], aw[0]));
        } else {
            NCT_HIP(hipMemcpyAsync(ann_prev, ann, sizeof(uint32_t) * ah[l - 1] * aw[l - 1], hipMemcpyDeviceToDevice, s));
            NCT_HIP(hipMemcpyAsync(bnn_prev, bnn, sizeof(uint32_t) * bh[l - 1] * bw[l - 1], hipMemcpyDeviceToDevice, s));
            NCT_TRY(nctk_nnf_upsample(ctx, s, ann_prev, ann, ah[l], aw[l], bh[l], bw[l], ah[l - 1], aw[l - 1]));
            NCT_TRY(nctk_nnf_upsample(ctx, s, bnn_prev, bnn, bh[l], bw[l], ah[l], aw[l], bh[l - 1], bw[l - 1]));
        }
        // normalise (main.cu:259-275), PatchMatch both directions (main.cu:283-284); S's normalised features serve every reference
        if (l > 0 && k == 0) NCT_TRY(nctk_normalize(ctx, s, sfeat, na, nullptr, C, na_px, feat16 ? (uint16_t*)na_h : nullptr));
        NCT_TRY(nctk_normalize(ctx, s, R[k].featp[l], nb, nullptr, C, nb_px, feat16 ? (uint16_t*)nb_h : nullptr));
        MARK(NCT_ST_OTHER, l);
        const uint32_t seed_ab = prm->seed ^ (0x9E3779B9u * (uint32_t)(2 * l + 1)), seed_ba = prm->seed ^ (0x9E3779B9u * (uint32_t)(2 * l + 2));
        const int pm_mode = (feat16 && C >= 256) ? NCT_PM_FP16 : NCT_PM_ROWREJECT;
        // SPEC §6.23 rules 5-6 (a frame of a carrying sequence that holds kept fields; false everywhere else): the kept fields of this reference follow the level's field,
        // then replace the start field where their step-0 distance is strictly smaller; annd / bnnd take d_Z and are PatchMatch's to overwrite. The level then runs
        // carry_iters iterations. Both count as PatchMatch time
        const int pm_it = carry_merge ? seq_carry_iters(seq) : prm->pm_iters;
        if (carry_merge) {
            NCT_TRY(seq_carry_move(ctx, s, seq, l, k));
            NCT_TRY(nctk_nnf_merge(ctx, s, na, nb, (const uint16_t*)na_h, (const uint16_t*)nb_h, C, ah[l], aw[l], bh[l], bw[l], pm_mode, ann, seq->keep_ann[k][l], annd, nullptr,
                                   bnn, seq->keep_bnn[k][l], bnnd, nullptr));
        }
        // na, nb are unit vectors: the row-wise rejection is exact (and worth a third of the finest level: 15.7 vs 24.1 ms with NCT_PM_PLAIN). The fp16 tiles pay from C = 128 on (11-37 % per level); the C = 64 level is
        // latency bound, not byte bound (fp16 tiles: 15.8 vs 16.0 ms), and stays fp32
        NCT_TRY(nctk_patchmatch_bidir(ctx, s, na, nb, (const uint16_t*)na_h, (const uint16_t*)nb_h, C, ah[l], aw[l], bh[l], bw[l], pm_it, R[k].rs_range[l], seed_ab, seed_ba,
                                      ann, annd, bnn, bnnd, pm_mode, count ? ctx->d_counter + 4 * l : nullptr));
        if (carry_keep) {
            // SPEC §6.23 rule 1: the level's final fields are the sequence's kept fields from here on
            NCT_HIP(hipMemcpyAsync(seq->keep_ann[k][l], ann, sizeof(uint32_t) * na_px, hipMemcpyDeviceToDevice, s));
            NCT_HIP(hipMemcpyAsync(seq->keep_bnn[k][l], bnn, sizeof(uint32_t) * nb_px, hipMemcpyDeviceToDevice, s));
        }
        MARK(NCT_ST_PM, l);
        if (timing) timing->pm_level_launches[l] += 1 + 4 * pm_it;
        NCT_TRY(d2h(lv->ann[k][l], ann, sizeof(uint32_t) * na_px));
        NCT_TRY(d2h(lv->bnn[k][l], bnn, sizeof(uint32_t) * nb_px));
        NCT_TRY(d2h(lv->annd[k][l], annd, sizeof(float) * na_px));
        NCT_TRY(d2h(lv->bnnd[k][l], bnnd, sizeof(float) * nb_px));
        // BDS votes: guidance image (main.cu:291) and features + matching error (main.cu:303-318)
        // a masked reference (SPEC §6.12 rule 2; else qimg[l] is null): its level mask is pulled to S's grid behind the votes, through the same inversion of bnn
        NCT_TRY(nctk_bds_vote_both(ctx, s, R[k].img[l], R[k].featp[l], ann, bnn, C, ah[l], aw[l], bh[l], bw[l], 1.0, prm->bds_weight, guide_of(k), voted, R[k].qimg[l], R[k].pulled));
        NCT_TRY(nctk_normalize(ctx, s, voted, nvoted, nullptr, C, na_px));
        return nctk_feature_distance(ctx, s, na, nvoted, err_of(k), C, na_px);
    }
    // where reference k's guidance image and matching error go: with several references into its own maps, which the selection merges
    uint8_t* guide_of(int k) { return K > 1 ? R[k].guide : guide; }
    float* err_of(int k) { return K > 1 ? R[k].err : err; }

    // the correspondence of the level, once per reference in index order on the main stream (SPEC §6.2 rule 1; a pair runs the body once), then what the colour stage reads: G and E
    int correspondences(int l) {
        const int na_px = ah[l] * aw[l];
        field_found = false;
        if (carry_merge && seq->motion) {
            // SPEC §6.23 rule 2: the level's field in front of its correspondence, on the main stream, whether or not the frame blends; every later reader of the level
            // (the held selection, the held pull, the blend) uses this one
            DevBuf<uint8_t> lab_l(ctx, (size_t)na_px * 3);
            if (!lab_l.ok()) return NCT_ERR_HIP;
            NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], lab_l, (size_t)na_px));
            NCT_TRY(seq_motion_level(ctx, s, seq, l, lab_l));
            field_found = true;
        }
        for (int k = 0; k < K; ++k) {
            NCT_TRY(correspondence(l, k));
            if (K > 1 && k == K - 1) {
                // selection and merge (SPEC §6.2 rules 2-3): the one launch a level with several references adds; it counts as vote time
                const float* errs[NCT_MAX_REFS]; const uint8_t* guides[NCT_MAX_REFS];
                for (int q = 0; q < K; ++q) { errs[q] = R[q].err; guides[q] = R[q].guide; }
                if (held) NCT_TRY(held_selection(l, errs, guides));
                else NCT_TRY(nctk_select_reference(ctx, s, errs, guides, K, ah[l], aw[l], sel_label, guide, err));
                // a frame of a sequence keeps its label map (SPEC §6.18): the next full frame holds against it, a propagated frame carries it
                if (seq) NCT_HIP(hipMemcpyAsync(seq->keep_label[l], sel_label, (size_t)na_px, hipMemcpyDeviceToDevice, s));
            }
            if ((mask || ref_masked) && k == K - 1) NCT_TRY(level_masks(l));
            MARK(NCT_ST_VOTE, l);
            NCT_TRY(d2h(lv->ref_guide[k][l], guide_of(k), (size_t)na_px * 3));
            NCT_TRY(d2h(lv->ref_err[k][l], err_of(k), sizeof(float) * na_px));
        }
        // K = 1 has no selection: its label map is all zero and the merged maps are reference 0's
        if (K > 1) NCT_TRY(d2h(lv->label[l], sel_label, (size_t)na_px));
        else if (lv->label[l]) memset(lv->label[l], 0, (size_t)na_px);
        if (hlv && !held) {
            // a frame without a hold: the free label is the label, the margin 0.0
            if (K > 1) NCT_TRY(d2h(hlv->free_label[l], sel_label, (size_t)na_px));
            else if (hlv->free_label[l]) memset(hlv->free_label[l], 0, (size_t)na_px);
            if (hlv->margin[l]) std::fill(hlv->margin[l], hlv->margin[l] + na_px, 0.0);
        }
        NCT_TRY(d2h(lv->guide[l], guide, (size_t)na_px * 3));
        return d2h(lv->err[l], err, sizeof(float) * na_px);
    }

    // SPEC §6.18 rules 1-6 in the place of rule 2's launch. The rule reads L_t[l] and, with motion on, the level's field, which the level would otherwise find between S1
    // and the finish (seq_level_step): both are made here, on the main stream — the side stream's copy of L_t[l] has not been joined yet, and holds the same bytes —
    // and the blend then reads this field. The kept L_(t-1)[l], the packed map and the kept labels are still the previous frame's: the level replaces them behind S1
    int held_selection(int l, const float* const* errs, const uint8_t* const* guides) {
        const int h = ah[l], w = aw[l];
        const size_t n = (size_t)h * w;
        // a frame that also holds its pull (SPEC §6.19) reads the same L_t[l] and field behind this: the image then outlives the call, in hold_lab
        DevBuf<uint8_t> lab_own, free_l; DevBuf<double> margin_l;
        DevBuf<uint8_t>& lab_l = pull_hold ? hold_lab : lab_own;
        if (!lab_l.alloc(ctx, n * 3)) return NCT_ERR_HIP;
        if (hlv && hlv->free_label[l] && !free_l.alloc(ctx, n)) return NCT_ERR_HIP;
        if (hlv && hlv->margin[l] && !margin_l.alloc(ctx, n)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], lab_l, n));
        if (seq->motion && !field_found) { NCT_TRY(seq_motion_level(ctx, s, seq, l, lab_l)); field_found = true; }
        NCT_TRY(nctk_select_hold(ctx, s, errs, guides, K, h, w, seq->keep_label[l], lab_l, seq->keep_lab[l], seq->motion ? seq->field[l] : nullptr, seq->hold, seq->sigma,
                                 sel_label, guide, err, free_l, margin_l));
        if (free_l.ok()) NCT_TRY(dbg_copy(ctx, s, hlv->free_label[l], (uint8_t*)free_l, n));
        if (margin_l.ok()) NCT_TRY(dbg_copy(ctx, s, hlv->margin[l], (double*)margin_l, n));
        return NCT_OK;
    }

    // The level's mix mask m_l, behind the last reference's votes (and the selection). A source mask only (SPEC §6.11 rule 1): its level mask, no launch. With a reference mask
    // (SPEC §6.12 rules 3-4): P_l = the pulled mask of the pixel's label, M_l = min(P_l, the source's level mask) — one reference and no source mask: both are reference 0's
    // pulled mask, no launch
    int level_masks(int l) {
        if (!ref_masked) { m_l = mimg[l]; return NCT_OK; }
        const int na_px = ah[l] * aw[l];
        const uint8_t* pulled[NCT_MAX_REFS];
        for (int k = 0; k < K; ++k) pulled[k] = R[k].qimg[4] ? (const uint8_t*)R[k].pulled : nullptr;
        const uint8_t* p_free = K > 1 ? (const uint8_t*)p_merged : pulled[0];
        if (pull_hold) {
            // SPEC §6.19 rule 3: merge, hold and minimum in one launch, out of place into the sequence's second map; the two then change places. L_t[l] and (motion on) the
            // level's field are made here unless the held selection has made them; the blend reads that field. The kept L_(t-1)[l] is still the previous frame's
            const int h = ah[l], w = aw[l];
            if (!held) {
                if (!hold_lab.alloc(ctx, (size_t)na_px * 3)) return NCT_ERR_HIP;
                NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], hold_lab, (size_t)na_px));
                if (seq->motion && !field_found) { NCT_TRY(seq_motion_level(ctx, s, seq, l, hold_lab)); field_found = true; }
            }
            NCT_TRY(nctk_seq_pull_hold(ctx, s, pulled, K, sel_label, seq->keep_pull[l], hold_lab, seq->keep_lab[l], seq->motion ? seq->field[l] : nullptr, mask ? mimg[l] : nullptr, h, w,
                                       seq->tau, seq->sigma, seq->pull_alt[l], mask ? (uint8_t*)m_level : nullptr, p_merged.ok() ? (uint8_t*)p_merged : nullptr));
            hold_lab.reset();                                        // given back early, behind the hold
            seq->keep_pull[l].swap(seq->pull_alt[l]);
            p_l = seq->keep_pull[l];
            m_l = mask ? (const uint8_t*)m_level : p_l;
        } else {
            p_l = p_free;
            m_l = mask ? (const uint8_t*)m_level : p_l;
            if (K > 1 || mask) NCT_TRY(nctk_region_merge(ctx, s, pulled, K, sel_label, mimg[l], na_px, K > 1 ? (uint8_t*)p_merged : nullptr, mask ? (uint8_t*)m_level : nullptr));
            // a frame of a sequence that does not hold keeps P_l as its P' (SPEC §6.19 rule 3): a copy, no launch
            if (seq) NCT_HIP(hipMemcpyAsync(seq->keep_pull[l], p_l, (size_t)na_px, hipMemcpyDeviceToDevice, s));
        }
        if (plv) { NCT_TRY(d2h(plv->p_free[l], p_free, (size_t)na_px)); NCT_TRY(d2h(plv->p_held[l], p_l, (size_t)na_px)); }
        for (int k = 0; k < K && qlv; ++k) {
            if (!R[k].qimg[4]) continue;
            NCT_TRY(d2h(qlv->ref_mask[k][l], R[k].qimg[l], (size_t)R[k].bh[l] * R[k].bw[l]));
            NCT_TRY(d2h(qlv->pulled[k][l], R[k].pulled, (size_t)na_px));
        }
        return NCT_OK;
    }

    // level l's prebuilt part of S1's system with what the host knows about its hub blocks right now: the count, if the side stream has passed ev_level[l] (always, from
    // the second level on: the host has just waited for the previous level's WLS solve); else -1 and the hub pass is launched on the device-side count. The result does not depend on it.
    nct_s1_graph s1_graph_of(int l) {
        int hub_hint = -1, sup_hint = -1;
        // the coarsest level's graph is built while the host is still far ahead of the GPU (the VGG forwards are running), so its count has not arrived when the host gets
        // here: wait for that one event. The GPU has the level's correspondence work queued meanwhile and the solve's 200 launches are enqueued faster than they execute;
        // without the count the level's 101 hub passes (+ 101 second-level passes) would be launched blind (measured slower: DESIGN.md §9).
        if (ctx->s1_hub_hint && l == 0) (void)hipEventSynchronize(ctx->ev_level[0]);
        if (ctx->s1_hub_hint && hipEventQuery(ctx->ev_level[l]) == hipSuccess) { hub_hint = *(volatile int*)(ctx->s1_hub_blocks() + 2 * l); sup_hint = *(volatile int*)(ctx->s1_hub_blocks() + 2 * l + 1); }
        (void)hipGetLastError();                                     // hipEventQuery's hipErrorNotReady is not an error
        ctx->s1_hub_blocks_last[l] = hub_hint;
        return side.s1g[l].view(hub_hint, sup_hint);
    }

    // the colour stage of level l: the level's kNN graph joins from the side stream, local colour transfer (main.cu:368-380), the intermediate result in BGR
    int color_stage(int l) {
        const int na_px = ah[l] * aw[l];
        // kNN graph in Lab (main.cu:351-359): computed on the side stream; join once before its first use
        NCT_TRY(nctk_bgr2lab(ctx, s, guide, g_lab_l, na_px));
        if (l == 0) NCT_TRY(enqueue_side_graphs());
        NCT_HIP(hipStreamWaitEvent(s, ctx->ev_level[l], 0));          // level l's graph only: the fine levels keep overlapping
        if (l == nlevels - 1) ctx->flush_deferred();
        MARK(NCT_ST_KNN, l);
        ctx->tm_level = l;
        int wls_it[6] = {0, 0, 0, 0, 0, 0};
        nct_color_debug dbg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wls_it};
        const nct_color_stages* cs = color ? color[l] : nullptr;
        if (cs) { dbg.ab_local = cs->ab_local; dbg.ab_nonlocal = cs->ab_nonlocal; dbg.ab_up = cs->ab_up; dbg.rough = cs->roughness; dbg.ab_wls = cs->ab_wls; dbg.cg_iters = cs->cg_iters; }
        const nct_s1_graph s1graph = s1_graph_of(l);
        // the last level of a full-resolution run finishes on the original source; the exact finish converts S0 to Lab once, here (its time counts as colour stage)
        const full_target* const full = l == nlevels - 1 ? fin : nullptr;
        const nct_color_debug* const d = (timing || cs) ? &dbg : nullptr;
        full_lab fl; nct_color_bufs cb;
        NCT_TRY(fl.open(ctx, s, full));
        NCT_TRY(nctk_color_nonlocal(ctx, s, err, side.slab[l], g_lab_l, side.knn_ids[l], side.knn_ws[l], l, ah[l], aw[l], H, W, cp, cb, d, &s1graph));
        // a frame of a sequence: the blend between S1 and the finish, which then reads the kept X'_t (SPEC §6.3 rule 3)
        if (seq) NCT_TRY(seq_level_step(ctx, s, seq, l, side.slab[l], cb.x, cb.tmap, slv, field_found));
        // a masked run: S1's coefficients move toward the identity by the mix mask m_l, in place (SPEC §6.11 rule 2); the finish reads X' and composes with the source by f_l
        // (rule 3), the mask at the size the finish targets. A source mask only: f_l is that mask as it came. A masked frame of a sequence (SPEC §6.13 rule 2) mixes out of
        // place, from the kept X'_t into the level's own map, which the finish then reads: the state is never mixed. With a reference mask (SPEC §6.12 rules 4-5): F_l = P_l at that
        // size, then the minimum with the source's — the last level's is kept for nct_pair_fit_lut (rule 7)
        // (finish_level_masked; m_level, f_level and the map come from the run's own requests). Every level reports M_l, F_l and the mixed map
        if (mask || ref_masked) {
            masked_fin mf{ref_masked ? p_l : nullptr, mask ? mimg[l] : nullptr, mask, P->src, P->protect, l == nlevels - 1, m_l};
            NCT_TRY(finish_level_masked(ctx, s, mf, seq ? seq->keep_x[l] : (double*)cb.x, cb.x, m_level, f_level, P->fin_mask, ah[l], aw[l], H, W, s_lab_full, out_lab, P->out, full, fl,
                                        cp, d, nct_cube_form(*prm)));
            if (qlv) {
                NCT_TRY(dbg_copy(ctx, s, qlv->ab_mix[l], (double*)cb.x, (size_t)6 * na_px)); NCT_TRY(dbg_copy(ctx, s, qlv->mask[l], mf.m_l, (size_t)na_px));
                NCT_TRY(dbg_copy(ctx, s, qlv->mask_full[l], mf.f_l, (size_t)mf.fh * mf.fw));
            }
        } else NCT_TRY(finish_level(ctx, s, seq ? seq->keep_x[l] : (double*)cb.x, ah[l], aw[l], H, W, s_lab_full, out_lab, P->out, full, fl, cp, d, nct_cube_form(*prm)));
        if (cs && cs->wls_iters) for (int q = 0; q < 6; ++q) cs->wls_iters[q] = wls_it[q];
        if (timing) timing->wls_iters[l] = *std::max_element(wls_it, wls_it + 6);
        MARK(NCT_ST_COLOR, l);
        return d2h(lv->result[l], P->out, N * 3);
    }

    // re-predict: S features of the next level from the intermediate result (main.cu:424-427)
    int repredict(int l) {
        const int tap = 4 - l;                         // next level uses tap (5 - (l+1))
        float* taps_hwc[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        taps_hwc[tap - 1] = sfeat;
        NCT_TRY(nctk_vgg19_forward(ctx, s, P->out, H, W, W * 3, tap, nullptr, nullptr, taps_hwc));
        MARK(NCT_ST_VGG, l);
        return NCT_OK;
    }

    // everything the run enqueues, and the wait for the main stream. The side stream's kNN graphs (one per level that ran) finish before their buffers go back (~side_bufs)
    int run() {
        if (count) {
            if (!ctx->d_counter) NCT_HIP(hipMalloc(&ctx->d_counter, 32 * sizeof(unsigned long long)));
            NCT_HIP(hipMemsetAsync(ctx->d_counter, 0, 32 * sizeof(unsigned long long), s));
        }
        MARK(NCT_ST_OTHER, 0);
        geometry();
        NCT_TRY(lab_and_pyramids());
        NCT_TRY(forwards());
        if (refind) NCT_TRY(refind_masks());
        NCT_TRY(cluster());
        NCT_TRY(level_buffers());
        for (int l = 0; l < nlevels; ++l) {
            NCT_TRY(correspondences(l));
            NCT_TRY(color_stage(l));
            if (l < nlevels - 1) NCT_TRY(repredict(l));
        }
        NCT_HIP(hipStreamSynchronize(s));
        return NCT_OK;
    }
};

int process_resident(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const run_extras& x) {
    pair_state* P = (pair_state*)ctx->pair;
    if (P && P->seq && !x.seq) return ctx->fail(NCT_ERR_STATE, "process: a sequence is open on this context (nct_seq_frame runs its frames; nct_seq_end closes it)");
    if (!P || !P->src || P->K < 1 || !P->ref[0]) return ctx->fail(NCT_ERR_STATE, "process: no pair uploaded");
    NCT_REQUIRE(!x.fin || P->K == 1 || x.seq, "process: no full-resolution finish with several references");      // but for a frame of an open sequence (SPEC §6.18)
    NCT_REQUIRE(prm->patch_size == 3 && prm->k_num == 8, "process: patch_size must be 3 and k_num 8 (Config.h:68-70)");
    NCT_REQUIRE(prm->cluster_num >= 1 && prm->cluster_num <= 16, "process: cluster_num out of range");
    NCT_TRY(nct_params_check(ctx, "process", *prm));
    NCT_REQUIRE(prm->levels >= 1 && prm->levels <= 5, "process: levels must be in [1, 5] (got %d)", prm->levels);
    NCT_REQUIRE(!x.fin || ((!x.lv || x.seq) && !x.color), "process: no level intermediates with a full-resolution finish");     // a sequence's frame reports working-size maps only (nct_seq.cpp)
    NCT_REQUIRE(!x.color || P->K == 1 || x.seq, "process: nct_pair_levels describes a pair; several references report through nct_multi_levels");
    if (x.refusal) return ctx->fail(NCT_ERR_STATE, "%s", x.refusal);
    NCT_REQUIRE(!(P->mask && x.fin) || (x.fin->mask && (x.fin->finish == NCT_FINISH_EXACT || x.seq)), "process: a region mask is defined for the exact full-resolution finish only");
    NCT_REQUIRE(!(P->ref_masked() && x.fin) || x.fin->finish == NCT_FINISH_EXACT || x.seq, "process: a reference region mask is defined for the exact full-resolution finish only");
    // a new run on the resident images: an earlier full-resolution run is no longer the last one, and its two original-size images go back to the arena
    // (a full-resolution sequence keeps its two for its whole life: SPEC §6.9 rule 6)
    if (!(x.seq && x.seq->target())) {
        P->full_src.reset(); P->full_out.reset(); P->full_mask.reset();
    }
    P->fin_mask.reset();
    P->finished = false;
    run_clock clock(ctx, timing, prm->flags);
    pair_run run(ctx, prm, timing, x);
    const int rc = run.run();
    clock.stop();
    P->finished = rc == NCT_OK;
    return rc ? rc : clock.read(run.count);
}

nct_multi_levels multi_levels_of(const nct_pair_levels& levels) {
    nct_multi_levels m = {};
    for (int l = 0; l < 5; ++l) {
        m.ann[0][l] = levels.ann[l]; m.bnn[0][l] = levels.bnn[l]; m.annd[0][l] = levels.annd[l]; m.bnnd[0][l] = levels.bnnd[l];
        m.guide[l] = levels.guide[l]; m.err[l] = levels.err[l]; m.result[l] = levels.result[l];
    }
    m.labels = levels.labels;
    return m;
}
nct_ref_region_levels ref_region_levels_of(const nct_region_levels& levels) {
    nct_ref_region_levels q = {};
    for (int l = 0; l < 5; ++l) { q.ab_mix[l] = levels.ab_mix[l]; q.mask[l] = levels.mask[l]; }
    return q;
}

// SPEC §6.1 rule 1 (host/main.cpp's shrink: the longer side becomes max_side, the other (int)(max_side / (float)long * short)) and the limits of rule 5
const char* nct_working_size_rule(int h, int w, int max_side, int* work_h, int* work_w) {
    if (!work_h || !work_w) return "null output pointer";
    if (max_side < 17 || max_side > 4000) return "max_side must be in [17, 4000]";
    if (h < 1 || w < 1) return "image sides must be positive";
    if (h > NCT_FINISH_MAX_SIDE || w > NCT_FINISH_MAX_SIDE) return "image sides must be at most 16384";
    if ((long long)h * w > NCT_FINISH_MAX_PIXELS) return "images must have at most 2^26 pixels";
    int ch = h, cw = w;
    if (w > max_side || h > max_side) {
        cw = max_side; ch = (int)(cw / (float)w * h);
        if (w < h) { ch = max_side; cw = (int)(ch / (float)h * w); }
    }
    if (ch < 17 || cw < 17) return "the working size has a side below 17";
    *work_h = ch; *work_w = cw;
    return nullptr;
}

// what replaces the context's images is refused while a sequence holds them (SPEC §6.3)
#define NCT_NO_OPEN_SEQ(what) do { if (ctx->pair && ((pair_state*)ctx->pair)->seq) \
    return ctx->fail(NCT_ERR_STATE, what ": a sequence is open on this context (nct_seq_end closes it)"); } while (0)

// the source and its K references (checked by the caller) into the arena
static int upload_images(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw) {
    pair_state* P = pair_of(ctx);
    drop_images(P);
    if (!P->src.alloc(ctx, (size_t)sh * sw * 3)) return NCT_ERR_HIP;
    for (int k = 0; k < K; ++k) if (!P->ref[k].alloc(ctx, (size_t)rh[k] * rw[k] * 3)) return NCT_ERR_HIP;
    NCT_H2D(P->src, src_bgr, (size_t)sh * sw * 3);
    for (int k = 0; k < K; ++k) NCT_H2D(P->ref[k], refs_bgr[k], (size_t)rh[k] * rw[k] * 3);
    NCT_SYNC();
    P->sh = sh; P->sw = sw; P->K = K;
    for (int k = 0; k < K; ++k) { P->rh[k] = rh[k]; P->rw[k] = rw[k]; }
    return NCT_OK;
}

// The run forms of the C ABI on the uploaded images, `who` for the refusal texts. Each form names the reports it was given: multi, or pair — a pair reports as the list of
// one reference, its colour stages beside it — and region or ref_region, which describe the same masked run (SPEC §6.11, §6.12) and are refused without their mask
struct run_form { const nct_multi_levels* multi = nullptr; const nct_pair_levels* pair = nullptr; const nct_region_levels* region = nullptr; const nct_ref_region_levels* ref_region = nullptr; };
static int run_resident(nct_ctx* ctx, const char* who, const nct_params* prm, nct_pair_timing* timing, const run_form& f = {}) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm, "%s: null params", who);
    const pair_state* P = (pair_state*)ctx->pair;
    run_extras x; nct_multi_levels m; nct_ref_region_levels q;
    x.lv = f.multi;
    if (f.pair) { m = multi_levels_of(*f.pair); x.lv = &m; x.color = f.pair->color; }
    x.qlv = f.ref_region;
    if (f.ref_region && !(P && P->ref_masked())) x.refusal = "process: reference region levels asked for, but no reference mask is set (nct_pair_set_ref_region first)";
    if (f.region) { q = ref_region_levels_of(*f.region); x.qlv = &q; }
    if (f.region && !(P && P->mask)) x.refusal = "process: region levels asked for, but no region mask is set (nct_pair_set_region first)";
    return process_resident(ctx, prm, timing, x);
}

// The working-size nct_process_* forms, `who` for the refusal text: `upload` (the caller's, which words the refusals of the images), the masks that are given (ref_masks and
// each of its K entries nullable), `run` and the download. protect is read only where a mask is given, and refused before anything is uploaded
template <typename Upload>
static int process_form(nct_ctx* ctx, const char* who, Upload upload, const uint8_t* src_mask, int K, const uint8_t* const* ref_masks, const nct_region_params* region,
                        int (*run)(nct_ctx*, const nct_params*, nct_pair_timing*), const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    if (!ctx) return NCT_ERR_INVALID;
    bool any = src_mask != nullptr;
    for (int k = 0; k < K && k < NCT_MAX_REFS && ref_masks; ++k) any = any || ref_masks[k];
    NCT_REQUIRE(!any || !region || region->protect == 0 || region->protect == 1, "%s: region protect must be 0 or 1 (got %d)", who, region ? region->protect : 0);
    NCT_TRY(upload());
    if (src_mask) NCT_TRY(nct_pair_set_region(ctx, src_mask, region));
    for (int k = 0; k < K && ref_masks; ++k) if (ref_masks[k]) NCT_TRY(nct_pair_set_ref_region(ctx, k, ref_masks[k], region));
    NCT_TRY(run(ctx, prm, timing));
    return nct_pair_download(ctx, out_bgr);
}

extern "C" {

int nct_pair_upload(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw) {
    NCT_CTX_ENTER();
    NCT_NO_OPEN_SEQ("pair_upload");
    NCT_REQUIRE(src_bgr && ref_bgr, "pair_upload: null image");
    // the coarsest pyramid level (four ceil-halvings) must be at least 2x2 (init_Ann_kernel scales by (bw-1)/(aw-1)): side >= 17
    NCT_REQUIRE(sh >= 17 && sw >= 17 && rh >= 17 && rw >= 17 && sh <= 4000 && sw <= 4000 && rh <= 4000 && rw <= 4000,
                "pair_upload: image sides must be in [17, 4000] (got %dx%d and %dx%d)", sw, sh, rw, rh);
    return upload_images(ctx, src_bgr, sh, sw, 1, &ref_bgr, &rh, &rw);
}

int nct_multi_upload(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw) {
    NCT_CTX_ENTER();
    NCT_NO_OPEN_SEQ("multi_upload");
    NCT_REQUIRE(K >= 1 && K <= NCT_MAX_REFS, "multi_upload: the number of references must be in [1, %d] (got %d)", NCT_MAX_REFS, K);
    NCT_REQUIRE(src_bgr && refs_bgr && rh && rw, "multi_upload: null pointer");
    NCT_REQUIRE(sh >= 17 && sw >= 17 && sh <= 4000 && sw <= 4000, "multi_upload: image sides must be in [17, 4000] (source: %dx%d)", sw, sh);
    for (int k = 0; k < K; ++k) {
        NCT_REQUIRE(refs_bgr[k], "multi_upload: reference %d is a null image", k);
        NCT_REQUIRE(rh[k] >= 17 && rw[k] >= 17 && rh[k] <= 4000 && rw[k] <= 4000, "multi_upload: image sides must be in [17, 4000] (reference %d: %dx%d)", k, rw[k], rh[k]);
    }
    return upload_images(ctx, src_bgr, sh, sw, K, refs_bgr, rh, rw);
}

int nct_multi_run(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing) { return run_resident(ctx, "multi_run", prm, timing); }
int nct_multi_run_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_multi_levels* levels) {
    run_form f; f.multi = levels;
    return run_resident(ctx, "multi_run_levels", prm, timing, f);
}
int nct_pair_run(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing) { return run_resident(ctx, "pair_run", prm, timing); }
int nct_pair_run_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels) {
    run_form f; f.pair = levels;
    return run_resident(ctx, "pair_run_levels", prm, timing, f);
}

int nct_process_pair(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, const nct_params* prm,
                     uint8_t* out_bgr, nct_pair_timing* timing) {
    return process_form(ctx, "process_pair", [&] { return nct_pair_upload(ctx, src_bgr, sh, sw, ref_bgr, rh, rw); }, nullptr, 1, nullptr, nullptr, nct_pair_run, prm, out_bgr, timing);
}
int nct_process_multi(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, const nct_params* prm,
                      uint8_t* out_bgr, nct_pair_timing* timing) {
    return process_form(ctx, "process_multi", [&] { return nct_multi_upload(ctx, src_bgr, sh, sw, K, refs_bgr, rh, rw); }, nullptr, K, nullptr, nullptr, nct_multi_run, prm, out_bgr, timing);
}

// ---- source region masks (SPEC §6.11)
void nct_region_params_default(nct_region_params* p) {
    if (!p) return;
    p->protect = 0;
}

// kind: where `mask` lives — the caller's memory (nct_pair_set_region) or the device (pair_set_region_dev)
static int pair_set_region_from(nct_ctx* ctx, const uint8_t* mask, const nct_region_params* region, hipMemcpyKind kind) {
    NCT_CTX_ENTER();
    NCT_NO_OPEN_SEQ("pair_set_region");
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->src || P->sh < 1) return ctx->fail(NCT_ERR_STATE, "pair_set_region: no source uploaded (nct_pair_upload or nct_multi_upload first)");
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "pair_set_region: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    // the images stay; what an earlier run left is no longer the result of these settings
    P->finished = false;
    if (!mask) {
        if (P->mask.ok()) { NCT_SYNC(); P->mask.reset(); }
        P->protect = 0;
        return NCT_OK;
    }
    if (!P->mask.reserve(ctx, (size_t)P->sh * P->sw)) return NCT_ERR_HIP;
    NCT_HIP(hipMemcpyAsync(P->mask, mask, (size_t)P->sh * P->sw, kind, ctx->stream));
    NCT_SYNC();
    P->protect = region ? region->protect : 0;
    return NCT_OK;
}
int nct_pair_set_region(nct_ctx* ctx, const uint8_t* mask, const nct_region_params* region) { return pair_set_region_from(ctx, mask, region, hipMemcpyHostToDevice); }

int nct_pair_run_region_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_region_levels* region_levels) {
    run_form f; f.pair = levels; f.region = region_levels;
    return run_resident(ctx, "pair_run_region_levels", prm, timing, f);
}

int nct_process_pair_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask, const uint8_t* ref_bgr, int rh, int rw, const nct_region_params* region,
                            const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return process_form(ctx, "process_pair_region", [&] { return nct_pair_upload(ctx, src_bgr, sh, sw, ref_bgr, rh, rw); }, mask, 1, nullptr, region, nct_pair_run, prm, out_bgr, timing);
}

// ---- reference region masks (SPEC §6.12)
int nct_pair_set_ref_region(nct_ctx* ctx, int k, const uint8_t* mask, const nct_region_params* region) {
    NCT_CTX_ENTER();
    NCT_NO_OPEN_SEQ("pair_set_ref_region");
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->src || P->sh < 1 || P->K < 1) return ctx->fail(NCT_ERR_STATE, "pair_set_ref_region: no references uploaded (nct_pair_upload or nct_multi_upload first)");
    NCT_REQUIRE(k >= 0 && k < P->K, "pair_set_ref_region: k = %d is not one of the %d uploaded references", k, P->K);
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "pair_set_ref_region: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    P->finished = false;
    const size_t n = (size_t)P->rh[k] * P->rw[k];
    if (!mask) {
        if (P->rmask[k].ok()) { NCT_SYNC(); P->rmask[k].reset(); }
    } else {
        if (!P->rmask[k].reserve(ctx, n)) return NCT_ERR_HIP;
        NCT_H2D(P->rmask[k], mask, n);
        NCT_SYNC();
    }
    if (region) P->protect = region->protect;
    return NCT_OK;
}

int nct_multi_run_ref_region_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_multi_levels* levels, const nct_ref_region_levels* region_levels) {
    run_form f; f.multi = levels; f.ref_region = region_levels;
    return run_resident(ctx, "multi_run_ref_region_levels", prm, timing, f);
}
int nct_pair_run_ref_region_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_ref_region_levels* region_levels) {
    run_form f; f.pair = levels; f.ref_region = region_levels;
    return run_resident(ctx, "pair_run_ref_region_levels", prm, timing, f);
}

int nct_process_multi_ref_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* src_mask, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw,
                                 const uint8_t* const* ref_masks, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return process_form(ctx, "process_multi_ref_region", [&] { return nct_multi_upload(ctx, src_bgr, sh, sw, K, refs_bgr, rh, rw); }, src_mask, K, ref_masks, region, nct_multi_run, prm,
                        out_bgr, timing);
}
int nct_process_pair_ref_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* src_mask, const uint8_t* ref_bgr, int rh, int rw, const uint8_t* ref_mask,
                                const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return process_form(ctx, "process_pair_ref_region", [&] { return nct_pair_upload(ctx, src_bgr, sh, sw, ref_bgr, rh, rw); }, src_mask, 1, &ref_mask, region, nct_pair_run, prm,
                        out_bgr, timing);
}

int nct_pair_download(nct_ctx* ctx, uint8_t* out_bgr) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->out) return ctx->fail(NCT_ERR_STATE, "pair_download: no result (call nct_pair_run first)");
    NCT_REQUIRE(out_bgr, "pair_download: null pointer");
    NCT_D2H(out_bgr, P->out, (size_t)P->sh * P->sw * 3);
    NCT_SYNC();
    return NCT_OK;
}

int nct_working_size(int h, int w, int max_side, int* work_h, int* work_w) {
    const char* why = nct_working_size_rule(h, w, max_side, work_h, work_w);
    if (why) { nct_set_ctxless_error(why); return NCT_ERR_INVALID; }
    return NCT_OK;
}

int nct_process_pair_fullres(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, int max_side,
                             const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return nct_process_pair_fullres_finish(ctx, src_bgr, sh, sw, ref_bgr, rh, rw, max_side, NCT_FINISH_EXACT, prm, out_bgr, timing);
}

// finish: NCT_FINISH_EXACT — the last level's U1 / S2 / A1 on the original source (SPEC §6.1); NCT_FINISH_UPSAMPLE — they stay at the working size and S2's output
// is upsampled onto the original source (SPEC §6.8)
int nct_process_pair_fullres_finish(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, int max_side, int finish,
                                    const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return nct_process_pair_fullres_finish_region(ctx, src_bgr, sh, sw, nullptr, ref_bgr, rh, rw, max_side, finish, nullptr, prm, out_bgr, timing);
}

int nct_process_pair_fullres_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, int max_side,
                                    const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return nct_process_pair_fullres_finish_region(ctx, src_bgr, sh, sw, mask0, ref_bgr, rh, rw, max_side, NCT_FINISH_EXACT, region, prm, out_bgr, timing);
}

static int fullres_run(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, const uint8_t* ref_mask0, int max_side,
                       int finish, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing);
// mask0 (nullable: the unmasked run, with its launches and arena requests): the source's region mask at sh x sw (SPEC §6.11 rule 5)
int nct_process_pair_fullres_finish_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, int max_side,
                                           int finish, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return fullres_run(ctx, src_bgr, sh, sw, mask0, ref_bgr, rh, rw, nullptr, max_side, finish, region, prm, out_bgr, timing);
}
// SPEC §6.12 rule 5: both masks at the original sizes, the exact finish
int nct_process_pair_fullres_ref_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, const uint8_t* ref_mask0,
                                        int max_side, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    return fullres_run(ctx, src_bgr, sh, sw, mask0, ref_bgr, rh, rw, ref_mask0, max_side, NCT_FINISH_EXACT, region, prm, out_bgr, timing);
}
// ref_mask0 (nullable): the reference's region mask at rh x rw (SPEC §6.12), shrunk with its image
static int fullres_run(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, const uint8_t* ref_mask0, int max_side,
                       int finish, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing) {
    NCT_CTX_ENTER();
    NCT_NO_OPEN_SEQ("process_pair_fullres");
    NCT_REQUIRE(src_bgr && ref_bgr && prm && out_bgr, "process_pair_fullres: null pointer");
    NCT_REQUIRE(finish == NCT_FINISH_EXACT || finish == NCT_FINISH_UPSAMPLE, "process_pair_fullres: finish must be NCT_FINISH_EXACT (0) or NCT_FINISH_UPSAMPLE (1) (got %d)", finish);
    NCT_REQUIRE(!mask0 || finish == NCT_FINISH_EXACT, "process_pair_fullres: a region mask with NCT_FINISH_UPSAMPLE is not defined (SPEC 6.11 rule 8): use NCT_FINISH_EXACT");
    NCT_REQUIRE((!mask0 && !ref_mask0) || !region || region->protect == 0 || region->protect == 1, "process_pair_fullres: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    int wh = 0, ww = 0, rwh = 0, rww = 0;
    const char* why = nct_working_size_rule(sh, sw, max_side, &wh, &ww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "process_pair_fullres: source %dx%d: %s", sw, sh, why);
    why = nct_working_size_rule(rh, rw, max_side, &rwh, &rww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "process_pair_fullres: reference %dx%d: %s", rw, rh, why);
    const bool shrunk = wh != sh || ww != sw;
    // the originals go to the arena and are shrunk there (rule 1: nct_resize_u8c3's arithmetic); the pair state holds the working-size pair
    pair_state* P = pair_of(ctx);
    drop_images(P);
    DevBuf<uint8_t> s0(ctx, (size_t)sh * sw * 3);
    if (!s0.ok()) return NCT_ERR_HIP;
    if (!P->src.alloc(ctx, (size_t)wh * ww * 3) || !P->ref[0].alloc(ctx, (size_t)rwh * rww * 3)) return NCT_ERR_HIP;
    P->sh = P->sw = P->rh[0] = P->rw[0] = 0;
    NCT_TRY(upload_shrunk(ctx, src_bgr, sh, sw, P->src, wh, ww, s0));
    NCT_TRY(upload_shrunk(ctx, ref_bgr, rh, rw, P->ref[0], rwh, rww));
    DevBuf<uint8_t> m0;
    if (mask0) {
        // rule 5: the mask arrives at the original size; the working mask is its single-channel resize (equal sizes: a copy)
        if (!m0.alloc(ctx, (size_t)sh * sw) || !P->mask.alloc(ctx, (size_t)wh * ww)) return NCT_ERR_HIP;
        NCT_H2D(m0, mask0, (size_t)sh * sw);
        NCT_TRY(nctk_resize_u8c1(ctx, ctx->stream, m0, sh, sw, P->mask, wh, ww));
        P->protect = region ? region->protect : 0;
    }
    DevBuf<uint8_t> q0;
    if (ref_mask0) {
        if (!q0.alloc(ctx, (size_t)rh * rw) || !P->rmask[0].alloc(ctx, (size_t)rwh * rww)) return NCT_ERR_HIP;
        NCT_H2D(q0, ref_mask0, (size_t)rh * rw);
        NCT_TRY(nctk_resize_u8c1(ctx, ctx->stream, q0, rh, rw, P->rmask[0], rwh, rww));
        P->protect = region ? region->protect : 0;
    }
    NCT_SYNC();
    P->sh = wh; P->sw = ww; P->rh[0] = rwh; P->rw[0] = rww; P->K = 1;
    if (!shrunk) {
        // rule 4: a source that is not shrunk has nothing to finish at another size — this is nct_process_pair on (S0, shrunk R)
        NCT_TRY(process_resident(ctx, prm, timing));
        return nct_pair_download(ctx, out_bgr);
    }
    DevBuf<uint8_t> o0(ctx, (size_t)sh * sw * 3);
    if (!o0.ok()) return NCT_ERR_HIP;
    const full_target fin{s0, sh, sw, o0, finish, m0};
    run_extras x; x.fin = &fin;
    const int rc = process_resident(ctx, prm, timing, x);
    // the working-size result buffer holds the second-to-last level's image (the upsampling finish: the working-size result, which nobody asked for): no nct_pair_download of it
    P->out.reset();
    if (rc) return rc;
    NCT_D2H(out_bgr, o0, (size_t)sh * sw * 3);
    NCT_SYNC();
    P->full_src.take(s0); P->full_out.take(o0); P->full_h = sh; P->full_w = sw;
    if (mask0) P->full_mask.take(m0);
    return NCT_OK;
}

// SPEC §6.6 rule 10: the table of the last finished run, from the images the context still holds on the device
int nct_pair_fit_lut(nct_ctx* ctx, const nct_lut_params* prm, float* lut_out) {
    NCT_CTX_ENTER();
    nct_lut_images im;
    if (!nct_pair_lut_images(ctx, &im)) return ctx->fail(NCT_ERR_STATE, "pair_fit_lut: no finished run on this context (nct_pair_run first)");
    NCT_TRY(nct_lut_fit_check(ctx, "pair_fit_lut", im.src, im.res, im.npix, prm, lut_out));
    const size_t n = (size_t)prm->size * prm->size * prm->size * 3;
    DevBuf<float> dl(ctx, n);
    if (!dl.ok()) return NCT_ERR_HIP;
    if (im.mask) NCT_TRY(nct_lut_fit_enqueue_masked(ctx, "pair_fit_lut", im.src, im.res, im.mask, im.npix, prm, dl, nullptr));
    else NCT_TRY(nct_lut_fit_enqueue(ctx, im.src, im.res, im.npix, prm, dl, nullptr));
    NCT_D2H(lut_out, dl, sizeof(float) * n);
    NCT_SYNC();
    return NCT_OK;
}

// SPEC §6.22 rule 7: the local colour grid of the last finished run, from the same images; a run's mask is not read (kept pixels fit a zero displacement)
int nct_pair_fit_grid(nct_ctx* ctx, const nct_grid_params* prm, double* grid_out) {
    NCT_CTX_ENTER();
    nct_lut_images im;
    if (!nct_pair_lut_images(ctx, &im)) return ctx->fail(NCT_ERR_STATE, "pair_fit_grid: no finished run on this context (nct_pair_run first)");
    NCT_TRY(nct_grid_fit_check(ctx, "pair_fit_grid", im.src, im.res, im.h, im.w, prm, grid_out));
    const size_t n = (size_t)prm->gy * prm->gx * prm->gz * 12;
    DevBuf<double> dg(ctx, n);
    if (!dg.ok()) return NCT_ERR_HIP;
    NCT_TRY(nct_grid_fit_enqueue(ctx, im.src, im.res, im.h, im.w, prm, dg, nullptr));
    NCT_D2H(grid_out, dg, sizeof(double) * n);
    NCT_SYNC();
    return NCT_OK;
}

}  // extern "C"

// what nct_pair_fit_lut and nct_lut_accum_add_run read: the source and the result of the last finished run, and the mask of a masked one
bool nct_pair_lut_images(nct_ctx* ctx, nct_lut_images* im) {
    pair_state* P = (pair_state*)ctx->pair;
    *im = nct_lut_images{nullptr, nullptr, nullptr, 0, 0, 0};
    if (!P || !P->finished) return false;
    // a masked run's table is fitted over its region (SPEC §6.11 rule 7), with the mask at the size of the images it reads
    if (P->full_src && P->full_out) *im = nct_lut_images{P->full_src, P->full_out, P->full_mask, (size_t)P->full_h * P->full_w, P->full_h, P->full_w};
    else if (P->src && P->out && P->sh > 0) *im = nct_lut_images{P->src, P->out, P->mask, (size_t)P->sh * P->sw, P->sh, P->sw};
    // a run with a reference mask: its last level's target mask, which has the size of the result (SPEC §6.12 rule 7)
    if (im->src && P->fin_mask) im->mask = P->fin_mask;
    return im->src != nullptr;
}

int pair_set_region_dev(nct_ctx* ctx, const uint8_t* d_mask, const nct_region_params* region) { return pair_set_region_from(ctx, d_mask, region, hipMemcpyDeviceToDevice); }
