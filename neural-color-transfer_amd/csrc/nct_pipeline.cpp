// nct_pipeline.cpp — the per-pair hot loop: the MI355X counterpart of transfer_color_single_bds (main.cu:47-454).
// Everything between "two BGR images in" and "one BGR image out" stays on the device: no per-level cudaMalloc/Free churn
// (main.cu:238-257,297-326), no D2H of NNFs/error maps (main.cu:286-289,318), no host-side BDS vote (main.cu:291),
// no CSR ping-pong for the solvers. S features are recomputed from the intermediate result only up to the tap the
// next level needs (1115 instead of 2297 GFLOP per 700x700 pair, identical values).
#include "nct_internal.h"
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <algorithm>
#include <cmath>

// An open frame sequence (SPEC §6.3): what nct_seq_begin prepares once and every frame borrows — the reference's pyramid and its five un-normalised taps (HWC, by
// level) — and the state the blend carries from frame to frame, per level X' ([2][h*w][3] doubles) and L (the frame's level image in 8-bit Lab). All of it comes from
// the context's arena and outlives the runs; the frame and the reference at working size are pair_state's src / ref[0] as for a pair.
// While motion compensation is on (SPEC §6.4, nct_seq_set_motion) it also holds, per level, L packed one word per pixel and the level's field (4 B per level pixel each).
// A propagated frame (SPEC §6.5) with motion on warps X' out of place: warp_x, one map of the largest level run, reserved by the first such frame.
// The two counters of the key-frame decision (SPEC §6.7 rule 3) are host integers: they cost no device memory.
// A full-resolution sequence (SPEC §6.9, nct_seq_begin_fullres) keeps all of that on the working-size grids and adds the frame at its original size H0 x W0 and
// its result: pair_state's full_src / full_out, which live as long as the sequence and are what nct_pair_fit_lut reads.
struct seq_state {
    nct_params prm; double tau = 0, sigma = 0;
    long frames = 0;                                           // frames since nct_seq_begin / nct_seq_reset: 0 = the next one is a first frame
    long gap = 0;                                              // propagated frames since the last full frame, whichever call ran them
    unsigned long long acc = 0;                                // sum of `changed` over the frames nct_seq_frame_auto propagated since the last full frame
    int ah[5], aw[5], bh[5], bw[5];
    uint8_t* rpyr[4] = {}; float* rfeat[5] = {};
    double* keep_x[5] = {}; uint8_t* keep_lab[5] = {};
    bool motion = false; nct_seq_motion mp = {0, 0, 0};
    uint32_t* keep_pk[5] = {}; int16_t* field[5] = {};
    double* warp_x = nullptr;
    bool fullres = false; int H0 = 0, W0 = 0, finish = NCT_FINISH_EXACT;
};
struct pair_state {
    uint8_t *src = nullptr, *out = nullptr;                    // device BGR images
    seq_state* seq = nullptr;
    uint8_t* ref[NCT_MAX_REFS] = {};                           // the K references (SPEC §6.2; a pair: K = 1)
    int K = 0;
    int sh = 0, sw = 0, rh[NCT_MAX_REFS] = {}, rw[NCT_MAX_REFS] = {};
    uint8_t *full_src = nullptr, *full_out = nullptr;          // a finished full-resolution run (SPEC §6.1): the original source and its result, full_h x full_w, kept for nct_pair_fit_lut
    int full_h = 0, full_w = 0;
    bool finished = false;                                     // the last run on these images ran to its end: `out` (or full_out) holds its result
};
static pair_state* pair_of(nct_ctx* ctx) {
    if (!ctx->pair) ctx->pair = new pair_state();
    return (pair_state*)ctx->pair;
}
// drop what the context holds of the last pair / reference list
static void drop_images(nct_ctx* ctx, pair_state* P) {
    if (P->src) { ctx->release(P->src); P->src = nullptr; }
    for (uint8_t*& r : P->ref) if (r) { ctx->release(r); r = nullptr; }
    if (P->out) { ctx->release(P->out); P->out = nullptr; }
    if (P->full_src) { ctx->release(P->full_src); P->full_src = nullptr; }
    if (P->full_out) { ctx->release(P->full_out); P->full_out = nullptr; }
    P->K = 0; P->finished = false;
}
// what motion compensation holds goes back to the arena
static void seq_motion_free(nct_ctx* ctx, seq_state* q) {
    for (int l = 0; l < 5; ++l) {
        if (q->keep_pk[l]) { ctx->release(q->keep_pk[l]); q->keep_pk[l] = nullptr; }
        if (q->field[l]) { ctx->release(q->field[l]); q->field[l] = nullptr; }
    }
    if (q->warp_x) { ctx->release(q->warp_x); q->warp_x = nullptr; }
    q->motion = false;
}
// what an open sequence holds goes back to the arena
static void seq_free(nct_ctx* ctx, pair_state* P) {
    seq_state* q = P->seq;
    if (!q) return;
    seq_motion_free(ctx, q);
    for (int l = 0; l < 5; ++l) {
        if (l < 4 && q->rpyr[l]) ctx->release(q->rpyr[l]);
        if (q->rfeat[l]) ctx->release(q->rfeat[l]);
        if (q->keep_x[l]) ctx->release(q->keep_x[l]);
        if (q->keep_lab[l]) ctx->release(q->keep_lab[l]);
    }
    delete q; P->seq = nullptr;
}
// the images live in the context arena like every other device buffer (no hipMalloc/hipFree — device-wide synchronisation points —
// between the pairs of other contexts in flight on the same GPU)
void nct_pair_free(nct_ctx* ctx) {
    if (!ctx->pair) return;
    seq_free(ctx, (pair_state*)ctx->pair);
    drop_images(ctx, (pair_state*)ctx->pair);
    delete (pair_state*)ctx->pair; ctx->pair = nullptr;
}

static const int kTapC[5] = {64, 128, 256, 512, 512};       // tap 1 (conv1_1) … tap 5 (conv5_1)

#define MARK(stage, level) NCT_TRY(ctx->mark(s, nct_stage_tag(stage, level)))

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

// what a finished run (the main stream has been synchronised) leaves for nct_pair_timing beside total_ms: the stage marks, the kernel clock, the evaluation counters
static int read_timing(nct_ctx* ctx, nct_pair_timing* timing, bool count) {
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

// the full-resolution finish of the last level (nct_process_pair_fullres, SPEC §6.1): the original source on the device and where its result goes
// finish: NCT_FINISH_EXACT moves U1 / S2 / A1 there, NCT_FINISH_UPSAMPLE leaves them at the working size and upsamples S2's output (SPEC §6.8)
struct fullres_target { const uint8_t* src; int H, W; uint8_t* out; int finish; };

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
    const fullres_target* const fin;               // nullable: moves the last level's U1 / S2 / A1 onto the original source
    seq_state* const seq;                          // nullable: this run is a frame of the open sequence (SPEC §6.3) — the reference's pyramid and taps are borrowed, S1's output is blended
    const nct_seq_levels* const slv;               // nullable: where a frame's X'_t and tau_p maps go
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
    const nct_color_params cp;

    pair_run(nct_ctx* c, const nct_params* p, nct_pair_timing* t, const nct_multi_levels* levels, const nct_color_stages* const* col, const fullres_target* f,
             seq_state* q = nullptr, const nct_seq_levels* sl = nullptr)
        : ctx(c), prm(p), timing(t), lv(levels ? levels : &kNoLevels), color(col), fin(f), seq(q), slv(sl), P((pair_state*)c->pair), s(c->stream), H(P->sh), W(P->sw), K(P->K),
          nlevels(p->levels), N((size_t)H * W), feat16((p->flags & NCT_FLAG_FEAT16) != 0), count(t && (p->flags & NCT_FLAG_COUNT_EVALS)), side(c),
          cp{p->eps, p->nonlocal_weight, p->local_weight, p->wls_lambda_init, p->wls_alpha, (double)p->k_num} {}

    int d2h(void* dst, const void* src, size_t bytes) {
        if (dst) NCT_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        return 0;
    }

    // level geometry, coarse -> fine (level 0 = conv5_1)
    void geometry() {
        { int h = H, w = W;
          for (int t = 0; t < 5; ++t) { ah[4 - t] = h; aw[4 - t] = w; h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; } }
        for (int k = 0; k < K; ++k) {
            int h2 = P->rh[k], w2 = P->rw[k];
            for (int t = 0; t < 5; ++t) { R[k].bh[4 - t] = h2; R[k].bw[4 - t] = w2; h2 = (h2 - 1) / 2 + 1; w2 = (w2 - 1) / 2 + 1; }
            // the random-search radius of reference k is the pair (S, R_k)'s own (SPEC §6.2 rule 1), not the largest reference's
            const int maxLen = std::max(std::max(W, H), std::max(P->rw[k], P->rh[k]));
            const int rs[5] = {maxLen / 16, maxLen / 32, maxLen / 64, 32, 32};                     // main.cu:77-83
            for (int l = 0; l < 5; ++l) R[k].rs_range[l] = rs[l];
            NR = std::max(NR, (size_t)P->rh[k] * P->rw[k]);
        }
    }

    // S in Lab (ColorTransfer ctor, ColorTransfer.h:54-75) and image pyramids (main.cu:104-108)
    int lab_and_pyramids() {
        if (!s_lab_full.alloc(ctx, N * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, P->src, s_lab_full, N));
        simg[4] = P->src;
        for (int k = 0; k < K; ++k) R[k].img[4] = P->ref[k];
        for (int l = 3; l >= 0; --l) {
            if (!spyr[l].alloc(ctx, (size_t)ah[l] * aw[l] * 3)) return NCT_ERR_HIP;
            for (int k = 0; k < K && !seq; ++k) if (!R[k].pyr[l].alloc(ctx, (size_t)R[k].bh[l] * R[k].bw[l] * 3)) return NCT_ERR_HIP;
            NCT_TRY(nctk_resize_u8c3(ctx, s, simg[l + 1], ah[l + 1], aw[l + 1], spyr[l], ah[l], aw[l]));
            simg[l] = spyr[l];
            if (seq) { R[0].img[l] = seq->rpyr[l]; continue; }          // the sequence's reference pyramid was built at nct_seq_begin
            for (int k = 0; k < K; ++k) {
                NCT_TRY(nctk_resize_u8c3(ctx, s, R[k].img[l + 1], R[k].bh[l + 1], R[k].bw[l + 1], R[k].pyr[l], R[k].bh[l], R[k].bw[l]));
                R[k].img[l] = R[k].pyr[l];
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
            for (int l = 0; l < 5; ++l) R[0].featp[l] = seq->rfeat[l];
            float* staps_hwc[5] = {nullptr, nullptr, nullptr, nullptr, sfeat};
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
        if (!P->out) { P->out = (uint8_t*)ctx->alloc(N * 3); if (!P->out) return NCT_ERR_HIP; }
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
        // na, nb are unit vectors: the row-wise rejection is exact (and worth a third of the finest level: 15.7 vs 24.1 ms with NCT_PM_PLAIN). The fp16 tiles pay from C = 128 on (11-37 % per level); the C = 64 level is
        // latency bound, not byte bound (fp16 tiles: 15.8 vs 16.0 ms), and stays fp32
        const int pm_mode = (feat16 && C >= 256) ? NCT_PM_FP16 : NCT_PM_ROWREJECT;
        NCT_TRY(nctk_patchmatch_bidir(ctx, s, na, nb, (const uint16_t*)na_h, (const uint16_t*)nb_h, C, ah[l], aw[l], bh[l], bw[l], prm->pm_iters, R[k].rs_range[l], seed_ab, seed_ba,
                                      ann, annd, bnn, bnnd, pm_mode, count ? ctx->d_counter + 4 * l : nullptr));
        MARK(NCT_ST_PM, l);
        if (timing) timing->pm_level_launches[l] += 1 + 4 * prm->pm_iters;
        NCT_TRY(d2h(lv->ann[k][l], ann, sizeof(uint32_t) * na_px));
        NCT_TRY(d2h(lv->bnn[k][l], bnn, sizeof(uint32_t) * nb_px));
        NCT_TRY(d2h(lv->annd[k][l], annd, sizeof(float) * na_px));
        NCT_TRY(d2h(lv->bnnd[k][l], bnnd, sizeof(float) * nb_px));
        // BDS votes: guidance image (main.cu:291) and features + matching error (main.cu:303-318)
        NCT_TRY(nctk_bds_vote_both(ctx, s, R[k].img[l], R[k].featp[l], ann, bnn, C, ah[l], aw[l], bh[l], bw[l], 1.0, prm->bds_weight, guide_of(k), voted));
        NCT_TRY(nctk_normalize(ctx, s, voted, nvoted, nullptr, C, na_px));
        return nctk_feature_distance(ctx, s, na, nvoted, err_of(k), C, na_px);
    }
    // where reference k's guidance image and matching error go: with several references into its own maps, which the selection merges
    uint8_t* guide_of(int k) { return K > 1 ? R[k].guide : guide; }
    float* err_of(int k) { return K > 1 ? R[k].err : err; }

    // the correspondence of the level, once per reference in index order on the main stream (SPEC §6.2 rule 1; a pair runs the body once), then what the colour stage reads: G and E
    int correspondences(int l) {
        const int na_px = ah[l] * aw[l];
        for (int k = 0; k < K; ++k) {
            NCT_TRY(correspondence(l, k));
            if (K > 1 && k == K - 1) {
                // selection and merge (SPEC §6.2 rules 2-3): the one launch a level with several references adds; it counts as vote time
                const float* errs[NCT_MAX_REFS]; const uint8_t* guides[NCT_MAX_REFS];
                for (int q = 0; q < K; ++q) { errs[q] = R[q].err; guides[q] = R[q].guide; }
                NCT_TRY(nctk_select_reference(ctx, s, errs, guides, K, ah[l], aw[l], sel_label, guide, err));
            }
            MARK(NCT_ST_VOTE, l);
            NCT_TRY(d2h(lv->ref_guide[k][l], guide_of(k), (size_t)na_px * 3));
            NCT_TRY(d2h(lv->ref_err[k][l], err_of(k), sizeof(float) * na_px));
        }
        // K = 1 has no selection: its label map is all zero and the merged maps are reference 0's
        if (K > 1) NCT_TRY(d2h(lv->label[l], sel_label, (size_t)na_px));
        else if (lv->label[l]) memset(lv->label[l], 0, (size_t)na_px);
        NCT_TRY(d2h(lv->guide[l], guide, (size_t)na_px * 3));
        return d2h(lv->err[l], err, sizeof(float) * na_px);
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
        nct_color_debug dbg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        int wls_it[6] = {0, 0, 0, 0, 0, 0};
        dbg.wls_iters = wls_it;
        const nct_color_stages* cs = color ? color[l] : nullptr;
        if (cs) { dbg.ab_local = cs->ab_local; dbg.ab_nonlocal = cs->ab_nonlocal; dbg.ab_up = cs->ab_up; dbg.rough = cs->roughness; dbg.ab_wls = cs->ab_wls; dbg.cg_iters = cs->cg_iters; }
        const nct_s1_graph s1graph = s1_graph_of(l);
        const int cube = (prm->flags & NCT_FLAG_LAB2BGR_CUBE) ? 1 : 0;
        // a frame of a sequence: the blend between S1 and the finish (SPEC §6.3 rule 3); the first frame and tau == 0 only keep the state, with no blend launch
        nct_seq_link link;
        if (seq) {
            link.keep_x = seq->keep_x[l]; link.keep_lab = seq->keep_lab[l]; link.blend = seq->frames > 0 && seq->tau > 0.0; link.tau = seq->tau; link.sigma = seq->sigma;
            link.ab_blend_host = slv ? slv->ab_blend[l] : nullptr; link.tau_map_host = slv ? slv->tau_map[l] : nullptr;
        }
        if (seq && seq->motion) {
            // SPEC §6.4: the first level run searches radius0 around (0, 0), every other level radius around twice the previous level's vector
            link.keep_pk = seq->keep_pk[l]; link.field = seq->field[l]; link.R = l == 0 ? seq->mp.radius0 : seq->mp.radius; link.penalty = seq->mp.penalty;
            if (l > 0) { link.parent = seq->field[l - 1]; link.ph = ah[l - 1]; link.pw = aw[l - 1]; }
            link.motion_host = slv ? slv->motion[l] : nullptr;
        }
        const bool last = l == nlevels - 1;
        if (fin && last && fin->finish == NCT_FINISH_EXACT) {
            // the last level finishes on the original source: S0 in Lab once, here (its time counts as colour stage), U1 / S2 / A1 at H0 x W0
            const size_t N0 = (size_t)fin->H * fin->W;
            DevBuf<uint8_t> s0_lab(ctx, N0 * 3), out0_lab(ctx, N0 * 3);
            if (!s0_lab.ok() || !out0_lab.ok()) return NCT_ERR_HIP;
            NCT_TRY(nctk_bgr2lab(ctx, s, fin->src, s0_lab, N0));
            const nct_finish_target ft{s0_lab, fin->H, fin->W, out0_lab};
            NCT_TRY(nctk_local_color_transfer(ctx, s, err, side.slab[l], g_lab_l, s_lab_full, side.knn_ids[l], side.knn_ws[l], l, ah[l], aw[l], H, W, cp, out_lab, timing ? &dbg : nullptr, &s1graph, &ft,
                                              seq ? &link : nullptr));
            NCT_TRY(nctk_lab2bgr(ctx, s, out0_lab, fin->out, N0, cube));
        } else {
            // the upsampling finish (SPEC §6.8): the last level finishes at the working size as ever, its S2 output then goes onto the original source
            const nct_finish_up up{fin ? fin->src : nullptr, fin ? fin->H : 0, fin ? fin->W : 0, fin ? fin->out : nullptr, cube};
            NCT_TRY(nctk_local_color_transfer(ctx, s, err, side.slab[l], g_lab_l, s_lab_full, side.knn_ids[l], side.knn_ws[l], l, ah[l], aw[l], H, W, cp, out_lab, (timing || cs) ? &dbg : nullptr, &s1graph,
                                              nullptr, seq ? &link : nullptr, (fin && last) ? &up : nullptr));
            if (cs && cs->wls_iters) for (int q = 0; q < 6; ++q) cs->wls_iters[q] = wls_it[q];
            NCT_TRY(nctk_lab2bgr(ctx, s, out_lab, P->out, N, cube));
        }
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

// run the whole L=5->1 loop on the uploaded source and its K references. lv (nullable): host copies of the level intermediates; color (nullable, a pair only): [5] the
// colour stage's coefficient maps per level; fin (nullable, a pair only): the full-resolution finish
static int process_resident(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_multi_levels* lv = nullptr, const nct_color_stages* const* color = nullptr,
                            const fullres_target* fin = nullptr, seq_state* seq = nullptr, const nct_seq_levels* slv = nullptr) {
    pair_state* P = (pair_state*)ctx->pair;
    if (P && P->seq && !seq) return ctx->fail(NCT_ERR_STATE, "process: a sequence is open on this context (nct_seq_frame runs its frames; nct_seq_end closes it)");
    if (!P || !P->src || P->K < 1 || !P->ref[0]) return ctx->fail(NCT_ERR_STATE, "process: no pair uploaded");
    NCT_REQUIRE(!fin || P->K == 1, "process: no full-resolution finish with several references");
    NCT_REQUIRE(prm->patch_size == 3 && prm->k_num == 8, "process: patch_size must be 3 and k_num 8 (Config.h:68-70)");
    NCT_REQUIRE(prm->cluster_num >= 1 && prm->cluster_num <= 16, "process: cluster_num out of range");
    NCT_REQUIRE(prm->levels >= 1 && prm->levels <= 5, "process: levels must be in [1, 5] (got %d)", prm->levels);
    NCT_REQUIRE(!fin || (!lv && !color), "process: no level intermediates with a full-resolution finish");
    NCT_REQUIRE(!color || P->K == 1, "process: nct_pair_levels describes a pair; several references report through nct_multi_levels");
    // a new run on the resident images: an earlier full-resolution run is no longer the last one, and its two original-size images go back to the arena
    // (a full-resolution sequence keeps its two for its whole life: SPEC §6.9 rule 6)
    if (!(seq && seq->fullres)) {
        if (P->full_src) { ctx->release(P->full_src); P->full_src = nullptr; }
        if (P->full_out) { ctx->release(P->full_out); P->full_out = nullptr; }
    }
    P->finished = false;
    if (timing) memset(timing, 0, sizeof *timing);
    auto wall0 = std::chrono::steady_clock::now();
    ctx->tm_on = timing != nullptr; ctx->tm_tags.clear(); ctx->tm_host.clear();
    ctx->kt_on = timing != nullptr && (prm->flags & NCT_FLAG_TIME_KERNELS) != 0; ctx->kt_ids.clear();
    ctx->wls_split = (prm->flags & NCT_FLAG_LATENCY) ? 1 : 0;
    pair_run run(ctx, prm, timing, lv, color, fin, seq, slv);
    const int rc = run.run();
    ctx->tm_on = false; ctx->kt_on = false;
    P->finished = rc == NCT_OK;
    if (rc || !timing) return rc;
    timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return read_timing(ctx, timing, run.count);
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
    drop_images(ctx, P);
    P->src = (uint8_t*)ctx->alloc((size_t)sh * sw * 3);
    if (!P->src) return NCT_ERR_HIP;
    for (int k = 0; k < K; ++k) { P->ref[k] = (uint8_t*)ctx->alloc((size_t)rh[k] * rw[k] * 3); if (!P->ref[k]) return NCT_ERR_HIP; }
    NCT_H2D(P->src, src_bgr, (size_t)sh * sw * 3);
    for (int k = 0; k < K; ++k) NCT_H2D(P->ref[k], refs_bgr[k], (size_t)rh[k] * rw[k] * 3);
    NCT_SYNC();
    P->sh = sh; P->sw = sw; P->K = K;
    for (int k = 0; k < K; ++k) { P->rh[k] = rh[k]; P->rw[k] = rw[k]; }
    return NCT_OK;
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

int nct_multi_run(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm, "multi_run: null params");
    return process_resident(ctx, prm, timing);
}

int nct_multi_run_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_multi_levels* levels) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm, "multi_run_levels: null params");
    return process_resident(ctx, prm, timing, levels);
}

int nct_process_multi(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, const nct_params* prm,
                      uint8_t* out_bgr, nct_pair_timing* timing) {
    NCT_TRY(nct_multi_upload(ctx, src_bgr, sh, sw, K, refs_bgr, rh, rw));
    NCT_TRY(nct_multi_run(ctx, prm, timing));
    return nct_pair_download(ctx, out_bgr);
}

int nct_pair_run(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm, "pair_run: null params");
    return process_resident(ctx, prm, timing);
}

int nct_pair_run_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm, "pair_run_levels: null params");
    if (!levels) return process_resident(ctx, prm, timing);
    // a pair is the list of one reference (SPEC §6.2): its maps are reference 0's NNFs and the merged guide / err; it has no label map and no G_k / E_k of their own
    nct_multi_levels m; memset(&m, 0, sizeof m);
    for (int l = 0; l < 5; ++l) {
        m.ann[0][l] = levels->ann[l]; m.bnn[0][l] = levels->bnn[l]; m.annd[0][l] = levels->annd[l]; m.bnnd[0][l] = levels->bnnd[l];
        m.guide[l] = levels->guide[l]; m.err[l] = levels->err[l]; m.result[l] = levels->result[l];
    }
    m.labels = levels->labels;
    return process_resident(ctx, prm, timing, &m, levels->color);
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

int nct_process_pair(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, const nct_params* prm,
                     uint8_t* out_bgr, nct_pair_timing* timing) {
    NCT_TRY(nct_pair_upload(ctx, src_bgr, sh, sw, ref_bgr, rh, rw));
    NCT_TRY(nct_pair_run(ctx, prm, timing));
    return nct_pair_download(ctx, out_bgr);
}

// ---- frame sequences (SPEC §6.3)
void nct_seq_params_default(nct_seq_params* p) {
    if (!p) return;
    p->tau = 0.7; p->sigma = 10.0;
}

int nct_seq_end(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->seq) return NCT_OK;
    NCT_SYNC();
    seq_free(ctx, P);
    drop_images(ctx, P);
    return NCT_OK;
}

void nct_seq_motion_default(nct_seq_motion* p) {
    if (!p) return;
    p->radius0 = 3; p->radius = 1; p->penalty = 1;
}

// SPEC §6.4: motion compensation of the open sequence on (from the next frame) or off. Turning it on reserves the packed maps and the fields and packs the kept L of
// a sequence that already has frames; turning it off gives them back
int nct_seq_set_motion(nct_ctx* ctx, const nct_seq_motion* mp) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->seq) return ctx->fail(NCT_ERR_STATE, "seq_set_motion: no sequence is open (nct_seq_begin first)");
    seq_state* q = P->seq;
    if (mp) {
        NCT_REQUIRE(mp->radius0 >= 0 && mp->radius0 <= 8, "seq_set_motion: radius0 must be in [0, 8] (got %d)", mp->radius0);
        NCT_REQUIRE(mp->radius >= 0 && mp->radius <= 3, "seq_set_motion: radius must be in [0, 3] (got %d)", mp->radius);
        NCT_REQUIRE(mp->penalty >= 0 && mp->penalty <= 255, "seq_set_motion: penalty must be in [0, 255] (got %d)", mp->penalty);
    }
    const bool on = mp && (mp->radius0 > 0 || mp->radius > 0);
    if (!on) {
        if (q->motion) { NCT_SYNC(); seq_motion_free(ctx, q); }
        return NCT_OK;
    }
    q->mp = *mp;
    if (q->motion) return NCT_OK;
    for (int l = 0; l < q->prm.levels; ++l) {
        const size_t n = (size_t)q->ah[l] * q->aw[l];
        q->keep_pk[l] = (uint32_t*)ctx->alloc(sizeof(uint32_t) * n); q->field[l] = (int16_t*)ctx->alloc(sizeof(int16_t) * 2 * n);
        if (!q->keep_pk[l] || !q->field[l]) { seq_motion_free(ctx, q); return NCT_ERR_HIP; }
    }
    q->motion = true;
    if (q->frames > 0) {
        for (int l = 0; l < q->prm.levels; ++l) {
            const int rc = nctk_seq_pack(ctx, ctx->stream, q->keep_lab[l], q->ah[l] * q->aw[l], q->keep_pk[l]);
            if (rc) { seq_motion_free(ctx, q); return rc; }
        }
    }
    return NCT_OK;
}

int nct_seq_reset(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->seq) return ctx->fail(NCT_ERR_STATE, "seq_reset: no sequence is open (nct_seq_begin first)");
    P->seq->frames = 0; P->seq->gap = 0; P->seq->acc = 0;
    return NCT_OK;
}

// the reference once: upload, pyramid (main.cu:104-108), one VGG19 forward with all five taps kept channel-last; and the per-level state
// rh0 x rw0: the reference as the caller holds it — larger than rh x rw only in a full-resolution sequence, which shrinks it on the device (SPEC §6.9)
static int seq_prepare(nct_ctx* ctx, pair_state* P, seq_state* q, const uint8_t* ref_bgr, int rh0, int rw0, int rh, int rw, int sh, int sw) {
    hipStream_t s = ctx->stream;
    { int h = sh, w = sw, h2 = rh, w2 = rw;
      for (int t = 0; t < 5; ++t) { q->ah[4 - t] = h; q->aw[4 - t] = w; q->bh[4 - t] = h2; q->bw[4 - t] = w2; h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; h2 = (h2 - 1) / 2 + 1; w2 = (w2 - 1) / 2 + 1; } }
    P->src = (uint8_t*)ctx->alloc((size_t)sh * sw * 3);
    P->ref[0] = (uint8_t*)ctx->alloc((size_t)rh * rw * 3);
    if (!P->src || !P->ref[0]) return NCT_ERR_HIP;
    P->sh = sh; P->sw = sw; P->K = 1; P->rh[0] = rh; P->rw[0] = rw;
    for (int l = 0; l < 5; ++l) {
        const size_t n = (size_t)q->ah[l] * q->aw[l], nr = (size_t)q->bh[l] * q->bw[l];
        if (l < 4 && !(q->rpyr[l] = (uint8_t*)ctx->alloc(nr * 3))) return NCT_ERR_HIP;
        if (!(q->rfeat[l] = (float*)ctx->alloc(sizeof(float) * kTapC[4 - l] * nr))) return NCT_ERR_HIP;
        if (l < q->prm.levels) {
            if (!(q->keep_x[l] = (double*)ctx->alloc(sizeof(double) * 6 * n)) || !(q->keep_lab[l] = (uint8_t*)ctx->alloc(n * 3))) return NCT_ERR_HIP;
        }
    }
    if (rh0 == rh && rw0 == rw) NCT_H2D(P->ref[0], ref_bgr, (size_t)rh * rw * 3);
    else {
        DevBuf<uint8_t> r0(ctx, (size_t)rh0 * rw0 * 3);
        if (!r0.ok()) return NCT_ERR_HIP;
        NCT_H2D(r0, ref_bgr, (size_t)rh0 * rw0 * 3);
        NCT_TRY(nctk_resize_u8c3(ctx, s, r0, rh0, rw0, P->ref[0], rh, rw));
    }
    if (q->fullres) {
        P->full_src = (uint8_t*)ctx->alloc((size_t)q->H0 * q->W0 * 3); P->full_out = (uint8_t*)ctx->alloc((size_t)q->H0 * q->W0 * 3);
        if (!P->full_src || !P->full_out) return NCT_ERR_HIP;
        P->full_h = q->H0; P->full_w = q->W0;
    }
    const uint8_t* img = P->ref[0];
    for (int l = 3; l >= 0; --l) {
        NCT_TRY(nctk_resize_u8c3(ctx, s, img, q->bh[l + 1], q->bw[l + 1], q->rpyr[l], q->bh[l], q->bw[l]));
        img = q->rpyr[l];
    }
    float* taps_hwc[5];
    for (int t = 0; t < 5; ++t) taps_hwc[t] = q->rfeat[4 - t];
    NCT_TRY(nctk_vgg19_forward(ctx, s, P->ref[0], rh, rw, rw * 3, 5, nullptr, nullptr, taps_hwc));
    NCT_SYNC();
    return NCT_OK;
}

int nct_seq_begin(nct_ctx* ctx, const uint8_t* ref_bgr, int rh, int rw, int sh, int sw, const nct_params* prm, const nct_seq_params* sp) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(ref_bgr && prm && sp, "seq_begin: null pointer");
    NCT_REQUIRE(sh >= 17 && sw >= 17 && rh >= 17 && rw >= 17 && sh <= 4000 && sw <= 4000 && rh <= 4000 && rw <= 4000,
                "seq_begin: image sides must be in [17, 4000] (got frames of %dx%d and a reference of %dx%d)", sw, sh, rw, rh);
    NCT_REQUIRE(sp->tau >= 0.0 && sp->tau < 1.0, "seq_begin: tau must be in [0, 1) (got %g)", sp->tau);
    NCT_REQUIRE(sp->sigma > 0.0 && sp->sigma <= 1.7976931348623157e308, "seq_begin: sigma must be finite and positive (got %g)", sp->sigma);
    NCT_REQUIRE(prm->levels >= 1 && prm->levels <= 5, "seq_begin: levels must be in [1, 5] (got %d)", prm->levels);
    NCT_TRY(nct_seq_end(ctx));                                   // a sequence that is still open is closed first
    pair_state* P = pair_of(ctx);
    drop_images(ctx, P);
    seq_state* q = new seq_state();
    q->prm = *prm; q->tau = sp->tau; q->sigma = sp->sigma;
    P->seq = q;
    const int rc = seq_prepare(ctx, P, q, ref_bgr, rh, rw, rh, rw, sh, sw);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); seq_free(ctx, P); drop_images(ctx, P); }
    return rc;
}

// SPEC §6.9: a sequence whose frames and reference arrive at their original size. Everything the sequence keeps lives on the working-size grids, as after
// nct_seq_begin on the shrunk images; only the last level's finish reaches the original frame
int nct_seq_begin_fullres(nct_ctx* ctx, const uint8_t* ref_bgr, int rh, int rw, int sh, int sw, int max_side, int finish, const nct_params* prm, const nct_seq_params* sp) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(ref_bgr && prm && sp, "seq_begin_fullres: null pointer");
    NCT_REQUIRE(finish == NCT_FINISH_EXACT || finish == NCT_FINISH_UPSAMPLE, "seq_begin_fullres: finish must be NCT_FINISH_EXACT (0) or NCT_FINISH_UPSAMPLE (1) (got %d)", finish);
    int wh = 0, ww = 0, rwh = 0, rww = 0;
    const char* why = nct_working_size_rule(sh, sw, max_side, &wh, &ww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "seq_begin_fullres: frames of %dx%d, max_side %d: %s", sw, sh, max_side, why);
    why = nct_working_size_rule(rh, rw, max_side, &rwh, &rww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "seq_begin_fullres: reference %dx%d, max_side %d: %s", rw, rh, max_side, why);
    NCT_REQUIRE(sp->tau >= 0.0 && sp->tau < 1.0, "seq_begin_fullres: tau must be in [0, 1) (got %g)", sp->tau);
    NCT_REQUIRE(sp->sigma > 0.0 && sp->sigma <= 1.7976931348623157e308, "seq_begin_fullres: sigma must be finite and positive (got %g)", sp->sigma);
    NCT_REQUIRE(prm->levels >= 1 && prm->levels <= 5, "seq_begin_fullres: levels must be in [1, 5] (got %d)", prm->levels);
    NCT_TRY(nct_seq_end(ctx));                                   // a sequence that is still open is closed first
    pair_state* P = pair_of(ctx);
    drop_images(ctx, P);
    seq_state* q = new seq_state();
    q->prm = *prm; q->tau = sp->tau; q->sigma = sp->sigma;
    q->fullres = true; q->H0 = sh; q->W0 = sw; q->finish = finish;
    P->seq = q;
    const int rc = seq_prepare(ctx, P, q, ref_bgr, rh, rw, rwh, rww, wh, ww);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); seq_free(ctx, P); drop_images(ctx, P); }
    return rc;
}

// a frame of the open sequence onto the device: into P->src, or (SPEC §6.9) at its original size into full_src and from there shrunk into P->src
static int seq_upload_frame(nct_ctx* ctx, pair_state* P, seq_state* q, const uint8_t* src_bgr) {
    if (!q->fullres) { NCT_H2D(P->src, src_bgr, (size_t)P->sh * P->sw * 3); return NCT_OK; }
    NCT_H2D(P->full_src, src_bgr, (size_t)q->H0 * q->W0 * 3);
    return nctk_resize_u8c3(ctx, ctx->stream, P->full_src, q->H0, q->W0, P->src, P->sh, P->sw);
}

int nct_seq_frame_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_seq_levels* seq_levels) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->seq) return ctx->fail(NCT_ERR_STATE, "seq_frame: no sequence is open (nct_seq_begin first)");
    NCT_REQUIRE(src_bgr && out_bgr, "seq_frame: null image");
    seq_state* q = P->seq;
    NCT_REQUIRE(!(q->fullres && levels), "seq_frame_levels: levels must be NULL in a full-resolution sequence (its result[] arrays have no single size); seq_levels reports the working-size maps");
    // a level without a field (motion off, a first frame, tau == 0) reports zeros
    if (seq_levels) for (int l = 0; l < q->prm.levels; ++l) if (seq_levels->motion[l]) memset(seq_levels->motion[l], 0, sizeof(int16_t) * 2 * (size_t)q->ah[l] * q->aw[l]);
    int rc = seq_upload_frame(ctx, P, q, src_bgr);
    nct_multi_levels m; memset(&m, 0, sizeof m);
    if (levels) {
        for (int l = 0; l < 5; ++l) {
            m.ann[0][l] = levels->ann[l]; m.bnn[0][l] = levels->bnn[l]; m.annd[0][l] = levels->annd[l]; m.bnnd[0][l] = levels->bnnd[l];
            m.guide[l] = levels->guide[l]; m.err[l] = levels->err[l]; m.result[l] = levels->result[l];
        }
        m.labels = levels->labels;
    }
    const fullres_target fin{P->full_src, q->H0, q->W0, P->full_out, q->finish};
    if (rc == NCT_OK) rc = process_resident(ctx, &q->prm, timing, levels ? &m : nullptr, levels ? levels->color : nullptr, q->fullres ? &fin : nullptr, q, seq_levels);
    // a frame that failed may have replaced the state of some levels only: the next frame starts over
    q->gap = 0; q->acc = 0;                                      // a full frame (and a failed one: the next is a first frame) starts the count over
    if (rc) { q->frames = 0; return rc; }
    q->frames += 1;
    if (!q->fullres) return nct_pair_download(ctx, out_bgr);
    NCT_D2H(out_bgr, P->full_out, (size_t)q->H0 * q->W0 * 3);
    NCT_SYNC();
    return NCT_OK;
}

int nct_seq_frame(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing) {
    return nct_seq_frame_levels(ctx, src_bgr, out_bgr, timing, nullptr, nullptr);
}

// SPEC §6.5: what a propagated frame enqueues — the frame's pyramid, per level L_t and (motion on) the field, the warp of the kept X' and the packed map, then the
// finish of the last level run on the kept X' and the frame's own pixels, and the download. Nothing upstream of the finish runs. L_t goes straight into the state:
// on this path nothing reads L_(t-1) but the search, which reads its packed form
static int propagate_run(nct_ctx* ctx, pair_state* P, seq_state* q, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* slv) {
    const hipStream_t s = ctx->stream;
    const nct_params& prm = q->prm;
    const int H = P->sh, W = P->sw, top = prm.levels - 1;
    const size_t N = (size_t)H * W;
    MARK(NCT_ST_OTHER, 0);
    DevBuf<uint8_t> s_lab_full(ctx, N * 3), out_lab(ctx, N * 3), spyr[4];
    if (!s_lab_full.ok() || !out_lab.ok()) return NCT_ERR_HIP;
    NCT_TRY(nctk_bgr2lab(ctx, s, P->src, s_lab_full, N));
    const uint8_t* simg[5]; simg[4] = P->src;
    for (int l = 3; l >= 0; --l) {
        if (!spyr[l].alloc(ctx, (size_t)q->ah[l] * q->aw[l] * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_resize_u8c3(ctx, s, simg[l + 1], q->ah[l + 1], q->aw[l + 1], spyr[l], q->ah[l], q->aw[l]));
        simg[l] = spyr[l];
    }
    MARK(NCT_ST_OTHER, 0);
    if (q->motion && !q->warp_x && !(q->warp_x = (double*)ctx->alloc(sizeof(double) * 6 * (size_t)q->ah[top] * q->aw[top]))) return NCT_ERR_HIP;
    if (!P->out) { P->out = (uint8_t*)ctx->alloc(N * 3); if (!P->out) return NCT_ERR_HIP; }
    for (int l = 0; l <= top; ++l) {
        const int h = q->ah[l], w = q->aw[l];
        const size_t n = (size_t)h * w;
        NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], q->keep_lab[l], n));
        if (q->motion) {
            NCT_TRY(nctk_seq_motion(ctx, s, q->keep_lab[l], q->keep_pk[l], h, w, l > 0 ? q->field[l - 1] : nullptr, l > 0 ? q->ah[l - 1] : 0, l > 0 ? q->aw[l - 1] : 0,
                                    l == 0 ? q->mp.radius0 : q->mp.radius, q->mp.penalty, q->field[l]));
            NCT_TRY(nctk_seq_warp(ctx, s, q->keep_x[l], h, w, q->field[l], q->warp_x));
            // the scratch has the last level's size: there the two maps change places, elsewhere the warped map is copied back
            if (l == top) std::swap(q->keep_x[l], q->warp_x);
            else NCT_HIP(hipMemcpyAsync(q->keep_x[l], q->warp_x, sizeof(double) * 6 * n, hipMemcpyDeviceToDevice, s));
            NCT_TRY(nctk_seq_pack(ctx, s, q->keep_lab[l], (int)n, q->keep_pk[l]));
        }
        if (slv) {
            if (slv->ab_blend[l]) NCT_HIP(hipMemcpyAsync(slv->ab_blend[l], q->keep_x[l], sizeof(double) * 6 * n, hipMemcpyDeviceToHost, s));
            if (slv->motion[l]) {
                if (q->motion) NCT_HIP(hipMemcpyAsync(slv->motion[l], q->field[l], sizeof(int16_t) * 2 * n, hipMemcpyDeviceToHost, s));
                else memset(slv->motion[l], 0, sizeof(int16_t) * 2 * n);
            }
            if (slv->tau_map[l]) std::fill(slv->tau_map[l], slv->tau_map[l] + n, 1.0);          // the previous frame's weight
        }
    }
    ctx->tm_level = top;
    int wls_it[6] = {0, 0, 0, 0, 0, 0};
    const nct_color_debug dbg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wls_it};
    const nct_color_params cp{prm.eps, prm.nonlocal_weight, prm.local_weight, prm.wls_lambda_init, prm.wls_alpha, (double)prm.k_num};
    const int cube = (prm.flags & NCT_FLAG_LAB2BGR_CUBE) ? 1 : 0;
    const size_t N0 = (size_t)q->H0 * q->W0;
    if (q->fullres && q->finish == NCT_FINISH_EXACT) {
        // SPEC §6.9 rule 3: the warped X' finishes on the original frame
        DevBuf<uint8_t> s0_lab(ctx, N0 * 3), out0_lab(ctx, N0 * 3);
        if (!s0_lab.ok() || !out0_lab.ok()) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, P->full_src, s0_lab, N0));
        NCT_TRY(nctk_color_finish(ctx, s, q->keep_x[top], q->ah[top], q->aw[top], H, W, s0_lab, q->H0, q->W0, cp, out0_lab, timing ? &dbg : nullptr));
        NCT_TRY(nctk_lab2bgr(ctx, s, out0_lab, P->full_out, N0, cube));
    } else {
        const nct_finish_up up{P->full_src, q->H0, q->W0, P->full_out, cube};
        NCT_TRY(nctk_color_finish(ctx, s, q->keep_x[top], q->ah[top], q->aw[top], H, W, s_lab_full, H, W, cp, out_lab, timing ? &dbg : nullptr, q->fullres ? &up : nullptr));
        NCT_TRY(nctk_lab2bgr(ctx, s, out_lab, P->out, N, cube));
    }
    if (timing) timing->wls_iters[top] = *std::max_element(wls_it, wls_it + 6);
    MARK(NCT_ST_COLOR, top);
    if (q->fullres) NCT_D2H(out_bgr, P->full_out, N0 * 3);
    else NCT_D2H(out_bgr, P->out, N * 3);
    NCT_SYNC();
    return NCT_OK;
}

int nct_seq_frame_propagate_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->seq) return ctx->fail(NCT_ERR_STATE, "seq_frame_propagate: no sequence is open (nct_seq_begin first)");
    seq_state* q = P->seq;
    if (q->frames == 0) return ctx->fail(NCT_ERR_STATE, "seq_frame_propagate: the sequence has no state to propagate (the first frame after nct_seq_begin / nct_seq_reset is nct_seq_frame's)");
    NCT_REQUIRE(src_bgr && out_bgr, "seq_frame_propagate: null image");
    if (timing) memset(timing, 0, sizeof *timing);
    const auto wall0 = std::chrono::steady_clock::now();
    ctx->tm_on = timing != nullptr; ctx->tm_tags.clear(); ctx->tm_host.clear();
    ctx->kt_on = timing != nullptr && (q->prm.flags & NCT_FLAG_TIME_KERNELS) != 0; ctx->kt_ids.clear();
    ctx->wls_split = (q->prm.flags & NCT_FLAG_LATENCY) ? 1 : 0;
    int rc = seq_upload_frame(ctx, P, q, src_bgr);
    if (rc == NCT_OK) rc = propagate_run(ctx, P, q, out_bgr, timing, seq_levels);
    ctx->tm_on = false; ctx->kt_on = false;
    // a frame that failed may have replaced the state of some levels only: the next frame starts over
    if (rc) { (void)hipStreamSynchronize(ctx->stream); q->frames = 0; q->gap = 0; q->acc = 0; return rc; }
    q->frames += 1; q->gap += 1;
    if (!timing) return NCT_OK;
    timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return read_timing(ctx, timing, false);
}

int nct_seq_frame_propagate(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing) {
    return nct_seq_frame_propagate_levels(ctx, src_bgr, out_bgr, timing, nullptr);
}

// ---- adaptive key frames (SPEC §6.7)
void nct_seq_auto_default(nct_seq_auto* p) {
    if (!p) return;
    p->threshold = 24; p->cut_permille = 500; p->key_permille = 100; p->max_gap = 8;
}

static const char* seq_auto_check(const nct_seq_auto& a) {
    if (a.threshold < 0 || a.threshold > 765) return "threshold must be in [0, 765]";
    if (a.cut_permille < 0 || a.cut_permille > 1001) return "cut_permille must be in [0, 1001]";
    if (a.key_permille < 0 || a.key_permille > 1001) return "key_permille must be in [0, 1001]";
    if (a.max_gap < 1 || a.max_gap > 1000) return "max_gap must be in [1, 1000]";
    return nullptr;
}

// SPEC §6.7 rule 3 on a measured frame: 64-bit integers, in this order. 1001 is "never": changed <= pixels makes the cut's comparison say so by itself; the accumulated
// count may exceed the pixels, so the key's 1001 is tested apart
static int seq_decide(const nct_seq_auto& a, const nct_seq_change_rec& c, unsigned long long acc, long gap) {
    const unsigned long long px = c.pixels;
    if ((unsigned long long)c.changed * 1000ull >= (unsigned long long)a.cut_permille * px) return NCT_SEQ_CUT;
    if (gap >= a.max_gap - 1 || (a.key_permille != 1001 && (acc + c.changed) * 1000ull >= (unsigned long long)a.key_permille * px)) return NCT_SEQ_KEY;
    return NCT_SEQ_PROPAGATED;
}

// SPEC §6.7 rule 2: what the probe enqueues — the frame into scratch (P->src may still be read by nct_pair_fit_lut), its pyramid, L_t[l] for l = 0 … lambda, with motion on
// the level's field against the kept packed map into the level's field buffer (scratch between frames), the measure at lambda, 16 bytes back. The kept L, the packed
// maps, X' and the counters are only read
static int probe_run(nct_ctx* ctx, pair_state* P, seq_state* q, const uint8_t* src_bgr, int threshold, int lambda, nct_seq_change_rec* rec) {
    const hipStream_t s = ctx->stream;
    const size_t N = (size_t)P->sh * P->sw;
    DevBuf<uint8_t> frame(ctx, N * 3), spyr[4], lab[3];
    DevBuf<nct_seq_change_rec> d_rec(ctx, 1);
    if (!frame.ok() || !d_rec.ok()) return NCT_ERR_HIP;
    if (q->fullres) {
        // SPEC §6.9: the original frame into scratch of its own size, shrunk from there
        DevBuf<uint8_t> frame0(ctx, (size_t)q->H0 * q->W0 * 3);
        if (!frame0.ok()) return NCT_ERR_HIP;
        NCT_H2D(frame0, src_bgr, (size_t)q->H0 * q->W0 * 3);
        NCT_TRY(nctk_resize_u8c3(ctx, s, frame0, q->H0, q->W0, frame, P->sh, P->sw));
    } else NCT_H2D(frame, src_bgr, N * 3);
    const uint8_t* simg[5]; simg[4] = frame;
    for (int l = 3; l >= 0; --l) {
        if (!spyr[l].alloc(ctx, (size_t)q->ah[l] * q->aw[l] * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_resize_u8c3(ctx, s, simg[l + 1], q->ah[l + 1], q->aw[l + 1], spyr[l], q->ah[l], q->aw[l]));
        simg[l] = spyr[l];
    }
    for (int l = 0; l <= lambda; ++l) {
        const int h = q->ah[l], w = q->aw[l];
        if (!lab[l].alloc(ctx, (size_t)h * w * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], lab[l], (size_t)h * w));
        if (q->motion)
            NCT_TRY(nctk_seq_motion(ctx, s, lab[l], q->keep_pk[l], h, w, l > 0 ? q->field[l - 1] : nullptr, l > 0 ? q->ah[l - 1] : 0, l > 0 ? q->aw[l - 1] : 0,
                                    l == 0 ? q->mp.radius0 : q->mp.radius, q->mp.penalty, q->field[l]));
    }
    NCT_TRY(nctk_seq_change(ctx, s, lab[lambda], q->keep_lab[lambda], q->ah[lambda], q->aw[lambda], q->motion ? q->field[lambda] : nullptr, threshold, d_rec));
    NCT_D2H(rec, d_rec, sizeof *rec);
    NCT_SYNC();
    return NCT_OK;
}

// the checks of nct_seq_probe / nct_seq_frame_auto, then the probe and the decision; first_ok: a sequence without state is NCT_SEQ_FIRST, not an error
static int seq_probe_decide(nct_ctx* ctx, const char* who, const uint8_t* src_bgr, const nct_seq_auto* a, bool first_ok, nct_seq_auto* used, nct_seq_decision* d) {
    pair_state* P = (pair_state*)ctx->pair;
    if (!P || !P->seq) return ctx->fail(NCT_ERR_STATE, "%s: no sequence is open (nct_seq_begin first)", who);
    seq_state* q = P->seq;
    if (q->frames == 0 && !first_ok)
        return ctx->fail(NCT_ERR_STATE, "%s: the sequence has no state to compare with (the first frame after nct_seq_begin / nct_seq_reset is nct_seq_frame's)", who);
    NCT_REQUIRE(src_bgr, "%s: null image", who);
    if (a) *used = *a; else nct_seq_auto_default(used);
    if (const char* why = seq_auto_check(*used)) return ctx->fail(NCT_ERR_INVALID, "%s: %s", who, why);
    memset(d, 0, sizeof *d);
    d->acc_changed = (uint32_t)std::min<unsigned long long>(q->acc, 0xffffffffull); d->gap = (int)q->gap;
    if (q->frames == 0) { d->kind = NCT_SEQ_FIRST; d->level = -1; return NCT_OK; }
    const auto wall0 = std::chrono::steady_clock::now();
    d->level = std::min(q->prm.levels - 1, 2);
    const int rc = probe_run(ctx, P, q, src_bgr, used->threshold, d->level, &d->change);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }     // the probe wrote no state: the sequence stays as it was
    d->probe_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    d->kind = seq_decide(*used, d->change, q->acc, q->gap);
    return NCT_OK;
}

int nct_seq_probe(nct_ctx* ctx, const uint8_t* src_bgr, const nct_seq_auto* a, nct_seq_decision* out) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(out, "seq_probe: null out");
    nct_seq_auto used; nct_seq_decision d;
    NCT_TRY(seq_probe_decide(ctx, "seq_probe", src_bgr, a, false, &used, &d));
    *out = d;
    return NCT_OK;
}

// SPEC §6.7 rule 4: probe, decide, one of the existing calls, the counters
int nct_seq_frame_auto(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_auto* a, nct_seq_decision* out) {
    NCT_CTX_ENTER();
    // refused before the probe runs; without an open sequence the state error below comes first, as in the other frame calls
    NCT_REQUIRE(!ctx->pair || !((pair_state*)ctx->pair)->seq || out_bgr, "seq_frame_auto: null image");
    nct_seq_auto used; nct_seq_decision d;
    NCT_TRY(seq_probe_decide(ctx, "seq_frame_auto", src_bgr, a, true, &used, &d));
    seq_state* q = ((pair_state*)ctx->pair)->seq;
    if (out) *out = d;
    if (d.kind == NCT_SEQ_PROPAGATED) {
        const unsigned long long acc = q->acc + d.change.changed;
        NCT_TRY(nct_seq_frame_propagate(ctx, src_bgr, out_bgr, timing));      // counts the frame in gap
        q->acc = acc;
        return NCT_OK;
    }
    if (d.kind == NCT_SEQ_CUT) NCT_TRY(nct_seq_reset(ctx));
    return nct_seq_frame(ctx, src_bgr, out_bgr, timing);                      // zeroes both counters
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
    NCT_CTX_ENTER();
    NCT_NO_OPEN_SEQ("process_pair_fullres");
    NCT_REQUIRE(src_bgr && ref_bgr && prm && out_bgr, "process_pair_fullres: null pointer");
    NCT_REQUIRE(finish == NCT_FINISH_EXACT || finish == NCT_FINISH_UPSAMPLE, "process_pair_fullres: finish must be NCT_FINISH_EXACT (0) or NCT_FINISH_UPSAMPLE (1) (got %d)", finish);
    int wh = 0, ww = 0, rwh = 0, rww = 0;
    const char* why = nct_working_size_rule(sh, sw, max_side, &wh, &ww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "process_pair_fullres: source %dx%d: %s", sw, sh, why);
    why = nct_working_size_rule(rh, rw, max_side, &rwh, &rww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "process_pair_fullres: reference %dx%d: %s", rw, rh, why);
    const bool shrunk = wh != sh || ww != sw;
    // the originals go to the arena and are shrunk there (rule 1: nct_resize_u8c3's arithmetic); the pair state holds the working-size pair
    pair_state* P = pair_of(ctx);
    drop_images(ctx, P);
    DevBuf<uint8_t> s0(ctx, (size_t)sh * sw * 3);
    if (!s0.ok()) return NCT_ERR_HIP;
    P->src = (uint8_t*)ctx->alloc((size_t)wh * ww * 3);
    P->ref[0] = (uint8_t*)ctx->alloc((size_t)rwh * rww * 3);
    if (!P->src || !P->ref[0]) return NCT_ERR_HIP;
    P->sh = P->sw = P->rh[0] = P->rw[0] = 0;
    NCT_H2D(s0, src_bgr, (size_t)sh * sw * 3);
    NCT_TRY(nctk_resize_u8c3(ctx, ctx->stream, s0, sh, sw, P->src, wh, ww));
    {
        DevBuf<uint8_t> r0(ctx, (size_t)rh * rw * 3);
        if (!r0.ok()) return NCT_ERR_HIP;
        NCT_H2D(r0, ref_bgr, (size_t)rh * rw * 3);
        NCT_TRY(nctk_resize_u8c3(ctx, ctx->stream, r0, rh, rw, P->ref[0], rwh, rww));
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
    const fullres_target fin{s0, sh, sw, o0, finish};
    const int rc = process_resident(ctx, prm, timing, nullptr, nullptr, &fin);
    // the working-size result buffer holds the second-to-last level's image (the upsampling finish: the working-size result, which nobody asked for): no nct_pair_download of it
    if (P->out) { ctx->release(P->out); P->out = nullptr; }
    if (rc) return rc;
    NCT_D2H(out_bgr, o0, (size_t)sh * sw * 3);
    NCT_SYNC();
    P->full_src = s0.detach(); P->full_out = o0.detach(); P->full_h = sh; P->full_w = sw;
    return NCT_OK;
}

// SPEC §6.6 rule 10: the table of the last finished run, from the images the context still holds on the device
int nct_pair_fit_lut(nct_ctx* ctx, const nct_lut_params* prm, float* lut_out) {
    NCT_CTX_ENTER();
    pair_state* P = (pair_state*)ctx->pair;
    const uint8_t *src = nullptr, *res = nullptr; size_t npix = 0;
    if (P && !P->finished) P = nullptr;
    if (P && P->full_src && P->full_out) { src = P->full_src; res = P->full_out; npix = (size_t)P->full_h * P->full_w; }
    else if (P && P->src && P->out && P->sh > 0) { src = P->src; res = P->out; npix = (size_t)P->sh * P->sw; }
    if (!src) return ctx->fail(NCT_ERR_STATE, "pair_fit_lut: no finished run on this context (nct_pair_run first)");
    NCT_TRY(nct_lut_fit_check(ctx, "pair_fit_lut", src, res, npix, prm, lut_out));
    const size_t n = (size_t)prm->size * prm->size * prm->size * 3;
    DevBuf<float> dl(ctx, n);
    if (!dl.ok()) return NCT_ERR_HIP;
    NCT_TRY(nct_lut_fit_enqueue(ctx, src, res, npix, prm, dl, nullptr));
    NCT_D2H(lut_out, dl, sizeof(float) * n);
    NCT_SYNC();
    return NCT_OK;
}

}  // extern "C"
