// nct_api.cpp — C-ABI entry points (host-pointer variants) + context / arena management.
// Every entry point here is a thin marshalling layer: upload, call the device launcher (nctk_*), download — the traffic and the blocks through one HostCall (nct_internal.h).
#include <atomic>
#include "nct_internal.h"
#include <chrono>
#include <cstring>
#include <cstdlib>
#include <mutex>

static std::string g_create_err;
void nct_set_ctxless_error(const char* msg) { g_create_err = msg; }   // the message of a failed entry point that takes no context (nct_last_error(NULL))
void nct_vgg_free(nct_ctx* ctx);   // nct_vgg.cpp

// NCT_ARENA_FILL: the whole block (its cached size, not the request) is set to the fill byte. Blocks are recycled in stream order over three streams, so the
// fill waits for every queued kernel that may still use the block and is complete before any stream touches it
static void* arena_filled(nct_ctx* c, void* p, size_t block_bytes) {
    if (c->arena_fill < 0) return p;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemset(p, c->arena_fill, block_bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { c->release(p); c->fail(NCT_ERR_HIP, "NCT_ARENA_FILL: filling a block of %zu bytes failed: %s", block_bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}

void* nct_ctx::alloc(size_t bytes) {
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    int best = -1;
    for (size_t i = 0; i < blocks.size(); ++i)
        if (!blocks[i].used && blocks[i].bytes >= bytes && (best < 0 || blocks[i].bytes < blocks[best].bytes)) best = (int)i;
    if (best >= 0 && blocks[best].bytes <= bytes * 2 + (1u << 20)) { blocks[best].used = true; return arena_filled(this, blocks[best].p, blocks[best].bytes); }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        // free cached-but-unused blocks and retry once
        for (auto& b : blocks) if (!b.used && b.p) { (void)hipFree(b.p); bytes_allocated -= b.bytes; b.p = nullptr; b.bytes = 0; }
        e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { fail(NCT_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return nullptr; }
    }
    bytes_allocated += bytes;
    for (auto& b : blocks) if (!b.p) { b = {p, bytes, true}; return arena_filled(this, p, bytes); }
    blocks.push_back({p, bytes, true});
    return arena_filled(this, p, bytes);
}
int nct_ctx::mark(hipStream_t s, int tag) {
    if (!tm_on) return 0;
    const size_t i = tm_tags.size();
    if (i >= tm_events.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return fail(NCT_ERR_HIP, "hipEventCreate failed");
        tm_events.push_back(e);
    }
    if (hipEventRecord(tm_events[i], s) != hipSuccess) return fail(NCT_ERR_HIP, "hipEventRecord failed");
    tm_tags.push_back(tag);
    tm_host.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count());
    return 0;
}
int nct_ctx::kt_begin(hipStream_t s, int id) {
    if (!kt_on) return 0;
    const size_t i = 2 * kt_ids.size();
    while (kt_events.size() < i + 2) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return fail(NCT_ERR_HIP, "hipEventCreate failed");
        kt_events.push_back(e);
    }
    if (hipEventRecord(kt_events[i], s) != hipSuccess) return fail(NCT_ERR_HIP, "hipEventRecord failed");
    kt_ids.push_back(id);
    return 0;
}
int nct_ctx::kt_end(hipStream_t s) {
    if (!kt_on || kt_ids.empty()) return 0;
    if (hipEventRecord(kt_events[2 * kt_ids.size() - 1], s) != hipSuccess) return fail(NCT_ERR_HIP, "hipEventRecord failed");
    return 0;
}
void nct_ctx::release(void* p) {
    if (defer_release) { deferred.push_back(p); return; }
    for (auto& b : blocks) if (b.p == p) { b.used = false; return; }
}

int nct_seq_blend_check(nct_ctx* ctx, const void* x, const void* x_prev, const void* lab, const void* lab_prev, int h, int w, const void* x_out, const void* field) {
    NCT_REQUIRE(x && x_prev && lab && lab_prev && x_out, "seq_blend: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_blend: grid %dx%d out of range", w, h);
    NCT_REQUIRE(!field || x_out != x_prev, "seq_blend: with a motion field x_out must not alias x_prev");
    return NCT_OK;
}
int nct_seq_motion_field_check(nct_ctx* ctx, const char* who, const void* lab, const void* lab_prev, int h, int w, const void* parent, int ph, int pw, const void* m_out) {
    NCT_REQUIRE(lab && lab_prev && m_out, "%s: null pointer", who);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "%s: grid %dx%d out of range", who, w, h);
    NCT_REQUIRE(!parent || (ph >= 1 && pw >= 1 && ph <= 4096 && pw <= 4096), "%s: parent grid %dx%d out of range", who, pw, ph);
    return NCT_OK;
}

extern "C" {

int nct_version(void) { return NCT_VERSION; }

int nct_create(int device, nct_ctx** out) {
    if (!out) { g_create_err = "nct_create: out is NULL"; return NCT_ERR_INVALID; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_err = std::string("nct_create: no usable HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                       "); libnct has no CPU fallback";
        return NCT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) { g_create_err = "nct_create: device index out of range"; return NCT_ERR_INVALID; }
    if ((e = hipSetDevice(device)) != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return NCT_ERR_HIP; }
    nct_ctx* c = new nct_ctx();
    c->device = device;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream_wls, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_wls_fork, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_wls_join, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming)) != hipSuccess) {
        g_create_err = std::string("stream/event creation: ") + hipGetErrorString(e);
        delete c; return NCT_ERR_HIP;
    }
    for (int l = 0; l < 5; ++l)
        if ((e = hipEventCreateWithFlags(&c->ev_level[l], hipEventDisableTiming)) != hipSuccess) { g_create_err = std::string("event creation: ") + hipGetErrorString(e); delete c; return NCT_ERR_HIP; }
    if ((e = hipHostMalloc(&c->pinned, 4096 + 64, hipHostMallocDefault)) != hipSuccess) { g_create_err = std::string("hipHostMalloc: ") + hipGetErrorString(e); delete c; return NCT_ERR_HIP; }
    if (const char* g = getenv("NCT_S2_LINES")) c->wls_lines = atoi(g) != 0;
    if (const char* f = getenv("NCT_WLS_FORECAST")) { const int v = atoi(f); if (v == 0 || v == 1) c->wls_forecast = v; }
    if (const char* r = getenv("NCT_WLS_RTOL")) { const double v = atof(r); if (v > 0 && v < 1) c->wls_rtol = v; }
    if (const char* f = getenv("NCT_CONV_POOL_FUSE")) { const int v = atoi(f); if (v == 0 || v == 1) c->conv_pool_fuse = v; }
    { static std::atomic<int> next_home{0}; c->home_xcd = next_home.fetch_add(1) & 7; }
    if (const char* q = getenv("NCT_CONV_PAIR")) { const int v = atoi(q); if (v == 0 || v == 1) c->conv_pair = v; }
    if (const char* q = getenv("NCT_KNN_RUNS")) { const int v = atoi(q); if (v == 0 || v == 1) c->knn_runs = v; }
    if (const char* q = getenv("NCT_S1_HUB_HINT")) { const int v = atoi(q); if (v == 0 || v == 1) c->s1_hub_hint = v; }
    if (const char* m = getenv("NCT_WLS_MAXIT")) { const int v = atoi(m); if (v > 0) c->wls_maxit = v; }
    c->wls_trace = getenv("NCT_WLS_TRACE") != nullptr;
    if (const char* m = getenv("NCT_S1_MAXIT")) { const int v = atoi(m); if (v > 0) c->s1_maxit = v; }
    if (const char* m = getenv("NCT_ARENA_FILL")) { char* end = nullptr; const long v = strtol(m, &end, 0); if (end != m && *end == 0 && v >= 0 && v <= 255) c->arena_fill = (int)v; }
    *out = c;
    return NCT_OK;
}

int nct_ctx_counter(nct_ctx* ctx, int which, int64_t* out) {
    if (!ctx || !out) return NCT_ERR_INVALID;
    switch (which) {
        case NCT_CTR_ARENA_BYTES: *out = (int64_t)ctx->bytes_allocated; return NCT_OK;
        case NCT_CTR_S1_HUB_BLOCKS_L0: case NCT_CTR_S1_HUB_BLOCKS_L0 + 1: case NCT_CTR_S1_HUB_BLOCKS_L0 + 2: case NCT_CTR_S1_HUB_BLOCKS_L0 + 3: case NCT_CTR_S1_HUB_BLOCKS_L0 + 4:
            *out = ctx->s1_hub_blocks_last[which - NCT_CTR_S1_HUB_BLOCKS_L0]; return NCT_OK;
    }
    return ctx->fail(NCT_ERR_INVALID, "nct_ctx_counter: unknown counter %d", which);
}

int nct_device_count(int* count) {
    if (!count) return NCT_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { *count = 0; g_create_err = "nct_device_count: no HIP device (no CPU fallback)"; return NCT_ERR_NO_DEVICE; }
    *count = n;
    return NCT_OK;
}
int nct_device_pci_bus_id(int device, char* buf, int buflen) {
    if (!buf || buflen < 13) return NCT_ERR_INVALID;
    hipError_t e = hipDeviceGetPCIBusId(buf, buflen, device);
    if (e != hipSuccess) { g_create_err = std::string("hipDeviceGetPCIBusId: ") + hipGetErrorString(e); return NCT_ERR_HIP; }
    for (char* p = buf; *p; ++p) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');      // sysfs spells the address in lower case
    return NCT_OK;
}

void nct_destroy(nct_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    nct_vgg_free(ctx);
    nct_cvt_free(ctx);
    nct_pair_free(ctx);
    nct_lut_accum_free(ctx);
    nct_reflib_ctx_free(ctx);
    for (auto& b : ctx->blocks) if (b.p) (void)hipFree(b.p);
    if (ctx->bench_a) (void)hipFree(ctx->bench_a);
    if (ctx->bench_b) (void)hipFree(ctx->bench_b);
    if (ctx->bench_ah16) (void)hipFree(ctx->bench_ah16);
    if (ctx->bench_bh16) (void)hipFree(ctx->bench_bh16);
    for (hipEvent_t e : ctx->tm_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->kt_events) (void)hipEventDestroy(e);
    if (ctx->d_counter) (void)hipFree(ctx->d_counter);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (int l = 0; l < 5; ++l) if (ctx->ev_level[l]) (void)hipEventDestroy(ctx->ev_level[l]);
    if (ctx->stream_wls) (void)hipStreamDestroy(ctx->stream_wls);
    if (ctx->ev_wls_fork) (void)hipEventDestroy(ctx->ev_wls_fork);
    if (ctx->ev_wls_join) (void)hipEventDestroy(ctx->ev_wls_join);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    delete ctx;
}

const char* nct_last_error(const nct_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int nct_device_name(nct_ctx* ctx, char* buf, int buflen) {
    if (!ctx || !buf || buflen <= 0) return NCT_ERR_INVALID;
    hipDeviceProp_t p;
    NCT_HIP(hipGetDeviceProperties(&p, ctx->device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return NCT_OK;
}

int nct_synchronize(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    NCT_HIP(hipDeviceSynchronize());
    return NCT_OK;
}


// The host-pointer entry points below, and those of nct_color.cpp, nct_lut.cpp, nct_grid.cpp, nct_region_select.cpp, nct_region_model.cpp and nct_vgg.cpp, have one shape: the argument
// checks; one HostCall line per array (in / out / inout / scratch, in the order the blocks are requested); NCT_TRY(hc.ready()) and the launchers; return hc.finish().

// a CHW host tensor through the staging block d_tmp (which several tensors of a call share) into HWC device layout
static int upload_hwc(nct_ctx* ctx, HostCall& hc, const float* chw, float* d_tmp, float* d_hwc, int C, int HW) {
    hc.put(d_tmp, chw, (size_t)C * HW);
    NCT_TRY(hc.ready());
    return nctk_chw_to_hwc(ctx, ctx->stream, d_tmp, d_hwc, C, HW);
}

int nct_feat_normalize(nct_ctx* ctx, const float* src_chw, float* dst_chw, float* resp, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(src_chw && dst_chw && H > 0 && W > 0, "feat_normalize: null pointer or empty image");
    const int HW = H * W; const size_t n = (size_t)C * HW;
    HostCall hc(ctx);
    float* t = hc.inout(src_chw, dst_chw, n);                  // Caffe's layout on the way in and on the way out
    float *x = hc.scratch<float>(n), *y = hc.scratch<float>(n), *r = hc.out(resp, HW);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_chw_to_hwc(ctx, ctx->stream, t, x, C, HW));
    NCT_TRY(nctk_normalize(ctx, ctx->stream, x, y, r, C, HW));
    NCT_TRY(nctk_hwc_to_chw(ctx, ctx->stream, y, t, C, HW));
    return hc.finish();
}

int nct_nnf_init(nct_ctx* ctx, uint32_t* nnf, int ah, int aw, int bh, int bw) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(nnf, "nnf_init: null pointer");
    NCT_REQUIRE(ah > 0 && aw > 0, "nnf_init: empty query image");
    HostCall hc(ctx);
    uint32_t* d = hc.out(nnf, (size_t)ah * aw);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_nnf_init(ctx, ctx->stream, d, ah, aw, bh, bw));
    return hc.finish();
}

int nct_nnf_upsample(nct_ctx* ctx, const uint32_t* nnf_half, uint32_t* nnf, int ah, int aw, int bh, int bw, int ah_half, int aw_half) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(nnf_half && nnf, "nnf_upsample: null pointer");
    NCT_REQUIRE(ah > 0 && aw > 0 && ah_half > 0 && aw_half > 0, "nnf_upsample: empty image");
    HostCall hc(ctx);
    const uint32_t* h = hc.in(nnf_half, (size_t)ah_half * aw_half);
    uint32_t* d = hc.out(nnf, (size_t)ah * aw);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_nnf_upsample(ctx, ctx->stream, h, d, ah, aw, bh, bw, ah_half, aw_half));
    return hc.finish();
}

int nct_patchmatch(nct_ctx* ctx, const float* a_chw, const float* b_chw, int C, int ah, int aw, int bh, int bw,
                   int patch, int iters, int rs_max, uint32_t seed, uint32_t* nnf, float* dist) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(a_chw && b_chw && nnf && dist, "patchmatch: null pointer");
    NCT_REQUIRE(patch == 3, "patchmatch: only patch=3 is supported (Config.h:70), got %d", patch);
    NCT_REQUIRE(ah > 0 && aw > 0 && bh > 0 && bw > 0, "patchmatch: empty image");
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    HostCall hc(ctx);
    float *t = hc.scratch<float>((size_t)C * (na > nb ? na : nb)), *A = hc.scratch<float>(C * na), *B = hc.scratch<float>(C * nb), *d = hc.out(dist, na);
    uint32_t* n = hc.inout(nnf, nnf, na);
    NCT_TRY(hc.ready());
    NCT_TRY(upload_hwc(ctx, hc, a_chw, t, A, C, (int)na));
    NCT_TRY(upload_hwc(ctx, hc, b_chw, t, B, C, (int)nb));
    NCT_TRY(nctk_patchmatch(ctx, ctx->stream, A, B, C, ah, aw, bh, bw, iters, rs_max, seed, n, d, nullptr));
    return hc.finish();
}

int nct_bds_vote_features(nct_ctx* ctx, const uint32_t* ann, const uint32_t* bnn, const float* pin_chw, float* pout_chw, float* pw,
                          int C, int ah, int aw, int bh, int bw, int patch, float w_coherence, float w_complete) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(ann && bnn && pin_chw && pout_chw, "bds_vote_features: null pointer");
    NCT_REQUIRE(patch == 3, "bds_vote_features: only patch=3 is supported, got %d", patch);
    NCT_REQUIRE(ah > 0 && aw > 0 && bh > 0 && bw > 0, "bds_vote_features: empty image");
    NCT_REQUIRE(C > 0 && (C & 3) == 0 && C <= 512, "bds_vote_features: C=%d must be a multiple of 4 and <= 512", C);      // nctk_bds_vote_features' own refusals, in front of the reservations
    NCT_REQUIRE(nct_nnf_dims_ok(ah, aw, bh, bw), "bds_vote_features: dims out of range (%dx%d vs %dx%d); NNF coordinates are 12-bit", ah, aw, bh, bw);
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    HostCall hc(ctx);
    float *t = hc.scratch<float>((size_t)C * (na > nb ? na : nb)), *P = hc.scratch<float>(C * nb), *O = hc.scratch<float>(C * na), *w = hc.out(pw, na);
    const uint32_t *da = hc.in(ann, na), *db = hc.in(bnn, nb);
    NCT_TRY(hc.ready());
    NCT_TRY(upload_hwc(ctx, hc, pin_chw, t, P, C, (int)nb));
    NCT_TRY(nctk_bds_vote_features(ctx, ctx->stream, da, db, P, O, w, C, ah, aw, bh, bw, w_coherence, w_complete));
    NCT_TRY(nctk_hwc_to_chw(ctx, ctx->stream, O, t, C, (int)na));
    hc.get(pout_chw, t, C * na);
    return hc.finish();
}

int nct_feature_distance(nct_ctx* ctx, const float* a_chw, const float* b_chw, float* err, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(a_chw && b_chw && err && H > 0 && W > 0, "feature_distance: null pointer or empty image");
    const size_t n = (size_t)H * W;
    HostCall hc(ctx);
    float *t = hc.scratch<float>(C * n), *A = hc.scratch<float>(C * n), *B = hc.scratch<float>(C * n), *e = hc.out(err, n);
    NCT_TRY(hc.ready());
    NCT_TRY(upload_hwc(ctx, hc, a_chw, t, A, C, (int)n));
    NCT_TRY(upload_hwc(ctx, hc, b_chw, t, B, C, (int)n));
    NCT_TRY(nctk_feature_distance(ctx, ctx->stream, A, B, e, C, (int)n));
    return hc.finish();
}

// What the two selections stage alike: the K error maps and — only where a merged guide is asked for — the K guidance images up, each list in one block, and the blocks
// of the outputs that were asked for. d.err / d.guide: the lists the launcher takes
struct select_blocks { const float* err[NCT_MAX_REFS]; const uint8_t* guide[NCT_MAX_REFS]; float* err_out; uint8_t *guide_out, *label; };
static void select_stage(HostCall& hc, const float* const* err, const uint8_t* const* guide_bgr, int K, size_t n, uint8_t* label, uint8_t* guide_out, float* err_out, select_blocks& d) {
    float* e = hc.scratch<float>(n * K);
    d.err_out = hc.out(err_out, n);
    uint8_t* g = guide_out ? hc.scratch<uint8_t>(n * 3 * K) : nullptr;
    d.guide_out = hc.out(guide_out, n * 3); d.label = hc.out(label, n);
    if (hc.ready() != NCT_OK) return;
    for (int k = 0; k < K; ++k) {
        d.err[k] = e + n * k; d.guide[k] = g ? g + n * 3 * k : nullptr;
        hc.put(e + n * k, err[k], n);
        if (g) hc.put(g + n * 3 * k, guide_bgr[k], n * 3);
    }
}

// SPEC §6.2 rules 2-3 on host maps: K error maps and guidance images up, one k_select_reference launch, label / merged guidance / merged error down
int nct_select_reference(nct_ctx* ctx, const float* const* err, const uint8_t* const* guide_bgr, int K, int h, int w, uint8_t* label, uint8_t* guide_out, float* err_out) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(K >= 1 && K <= NCT_MAX_REFS, "select_reference: K must be in [1, %d] (got %d)", NCT_MAX_REFS, K);
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "select_reference: grid %dx%d out of range", w, h);
    NCT_REQUIRE(err && (guide_bgr || !guide_out), "select_reference: null map list");
    for (int k = 0; k < K; ++k) NCT_REQUIRE(err[k] && (!guide_out || guide_bgr[k]), "select_reference: null map of reference %d", k);
    HostCall hc(ctx);
    select_blocks d;
    select_stage(hc, err, guide_bgr, K, (size_t)h * w, label, guide_out, err_out, d);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_select_reference(ctx, ctx->stream, d.err, guide_out ? d.guide : nullptr, K, h, w, d.label, d.guide_out, d.err_out));
    return hc.finish();
}

// SPEC §6.18 rules 1-6 on host maps: the K error maps and guidance images, the kept labels, the two Lab level images and the field up, one k_select_hold launch, the
// label, the merged maps, the free label and the margin down
int nct_select_reference_hold(nct_ctx* ctx, const float* const* err, const uint8_t* const* guide_bgr, int K, int h, int w, const uint8_t* prev_label, const uint8_t* lab,
                              const uint8_t* lab_prev, const int16_t* field, double hold, double sigma, uint8_t* label, uint8_t* guide_out, float* err_out,
                              uint8_t* free_label, double* margin) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_select_hold_check(ctx, "select_reference_hold", (const void* const*)err, (const void* const*)guide_bgr, K, h, w, prev_label, lab, lab_prev, hold, sigma, guide_out));
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    select_blocks d;
    select_stage(hc, err, guide_bgr, K, n, label, guide_out, err_out, d);
    const uint8_t* prev = hc.in(prev_label, n);
    uint8_t* fr = hc.out(free_label, n);
    const uint8_t *l1 = hc.in(lab, n * 3), *l0 = hc.in(lab_prev, n * 3);
    const int16_t* fld = hc.in(field, 2 * n);
    double* mg = hc.out(margin, n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_select_hold(ctx, ctx->stream, d.err, guide_out ? d.guide : nullptr, K, h, w, prev, l1, l0, fld, hold, sigma, d.label, d.guide_out, d.err_out, fr, mg));
    return hc.finish();
}

// SPEC §6.19 rules 2-4 on host maps: the pulled masks, the label map, the kept map, the two Lab level images, the field and the source mask up, one k_seq_pull_hold
// launch, P', M and the free P down
int nct_seq_pull_hold(nct_ctx* ctx, const uint8_t* const* pulled, int K, const uint8_t* label, const uint8_t* prev, const uint8_t* lab, const uint8_t* lab_prev,
                      const int16_t* field, const uint8_t* src_mask, int h, int w, double tau, double sigma, uint8_t* p_out, uint8_t* m_out, uint8_t* p_free) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_seq_pull_hold_check(ctx, "seq_pull_hold", (const void* const*)pulled, K, label, prev, lab, lab_prev, h, w, tau, sigma, p_out));
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    uint8_t* pk = hc.scratch<uint8_t>(n * K);                  // the K pulled masks in one block; a null one leaves its part unused
    const uint8_t *lbl = hc.in(label, n), *pv = hc.in(prev, n), *l1 = hc.in(lab, n * 3), *l0 = hc.in(lab_prev, n * 3), *ms = hc.in(src_mask, n);
    uint8_t *po = hc.out(p_out, n), *mo = hc.out(m_out, n), *pf = hc.out(p_free, n);
    const int16_t* fld = hc.in(field, 2 * n);
    NCT_TRY(hc.ready());
    const uint8_t* dp[NCT_MAX_REFS];
    for (int k = 0; k < K; ++k) {
        dp[k] = pulled[k] ? pk + n * k : nullptr;
        hc.put(pk + n * k, pulled[k], n);
    }
    NCT_TRY(nctk_seq_pull_hold(ctx, ctx->stream, dp, K, lbl, pv, l1, l0, fld, ms, h, w, tau, sigma, po, mo, pf));
    return hc.finish();
}

// SPEC §6.3 rule 3 on host maps: the two coefficient maps and the two Lab level images up, one k_seq_blend launch, X' (and the tau_p map) down
int nct_seq_blend(nct_ctx* ctx, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                  double* x_out, double* tau_map) {
    return nct_seq_blend_mc(ctx, x, x_prev, lab, lab_prev, h, w, tau, sigma, x_out, tau_map, nullptr);
}

// SPEC §6.4 rule 4 on host maps; without a field it is SPEC §6.3 rule 3. The two blend where a frame does: without a field in place into the previous state's copy,
// with one into S1's own map
int nct_seq_blend_mc(nct_ctx* ctx, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                     double* x_out, double* tau_map, const int16_t* field) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_seq_blend_check(ctx, x, x_prev, lab, lab_prev, h, w, x_out, field));
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    double *dx = hc.inout(x, field ? x_out : nullptr, 6 * n), *dp = hc.inout(x_prev, field ? nullptr : x_out, 6 * n), *dt = hc.out(tau_map, n);
    const uint8_t *dl = hc.in(lab, 3 * n), *dlp = hc.in(lab_prev, 3 * n);
    const int16_t* df = hc.in(field, 2 * n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_seq_blend(ctx, ctx->stream, dx, dp, dl, dlp, h, w, tau, sigma, field ? dx : dp, dt, df));
    return hc.finish();
}

// SPEC §6.4 rules 1-3 on host maps: the two Lab level images (and the coarser level's field) up, L_(t-1) packed, one k_seq_motion launch, the field down
int nct_seq_motion_field(nct_ctx* ctx, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, const int16_t* parent, int ph, int pw, int R, int penalty, int16_t* m_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_seq_motion_field_check(ctx, "seq_motion_field", lab, lab_prev, h, w, parent, ph, pw, m_out));
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    const uint8_t *dl = hc.in(lab, 3 * n), *dlp = hc.in(lab_prev, 3 * n);
    uint32_t* pk = hc.scratch<uint32_t>(n);
    const int16_t* dpar = hc.in(parent, 2 * (size_t)ph * pw);
    int16_t* dm = hc.out(m_out, 2 * n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_seq_pack(ctx, ctx->stream, dlp, (int)n, pk));
    NCT_TRY(nctk_seq_motion(ctx, ctx->stream, dl, pk, h, w, dpar, ph, pw, R, penalty, dm));
    return hc.finish();
}

// SPEC §6.5 rule 3 on host maps: the kept coefficients and the field up, one k_seq_warp launch out of place, the warped map down
int nct_seq_warp(nct_ctx* ctx, const double* x_prev, int h, int w, const int16_t* field, double* x_out) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(x_prev && field && x_out, "seq_warp: null pointer");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_warp: grid %dx%d out of range", w, h);
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    const double* dp = hc.in(x_prev, 6 * n);
    double* dx = hc.out(x_out, 6 * n);
    const int16_t* df = hc.in(field, 2 * n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_seq_warp(ctx, ctx->stream, dp, h, w, df, dx));
    return hc.finish();
}

// SPEC §6.14 rule 1 on host arrays: the matte and the field up, one k_seq_matte_warp launch out of place, the carried matte down
int nct_seq_matte_warp(nct_ctx* ctx, const uint8_t* mask_prev, int H, int W, const int16_t* field, int h, int w, uint8_t* mask_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_seq_matte_warp_check(ctx, "seq_matte_warp", mask_prev, H, W, field, h, w, mask_out));
    const size_t N = (size_t)H * W, n = (size_t)h * w;
    HostCall hc(ctx);
    const uint8_t* dp = hc.in(mask_prev, N);
    uint8_t* dm = hc.out(mask_out, N);
    const int16_t* df = hc.in(field, 2 * n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_seq_matte_warp(ctx, ctx->stream, dp, H, W, df, h, w, dm));
    return hc.finish();
}

// SPEC §6.23 rules 3, 4 and 6 on host arrays: the inputs up, the launches of the rule out of place, the output down
int nct_nnf_carry(nct_ctx* ctx, const uint32_t* nnf_prev, int h, int w, const int16_t* field, uint32_t* nnf_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_nnf_carry_check(ctx, "nnf_carry", nnf_prev, h, w, field, nnf_out));
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    const uint32_t* dp = hc.in(nnf_prev, n);
    const int16_t* df = hc.in(field, 2 * n);
    uint32_t* dout = hc.out(nnf_out, n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_nnf_carry(ctx, ctx->stream, dp, h, w, df, dout));
    return hc.finish();
}

int nct_nnf_forward_map(nct_ctx* ctx, const int16_t* field, int h, int w, uint32_t* fwd_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_nnf_forward_map_check(ctx, "nnf_forward_map", field, h, w, fwd_out));
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    const int16_t* df = hc.in(field, 2 * n);
    uint32_t* dout = hc.out(fwd_out, n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_nnf_forward_map(ctx, ctx->stream, df, h, w, dout));
    return hc.finish();
}

int nct_nnf_remap(nct_ctx* ctx, const uint32_t* bnn_prev, int bh, int bw, const uint32_t* fwd, int h, int w, uint32_t* bnn_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_nnf_remap_check(ctx, "nnf_remap", bnn_prev, bh, bw, fwd, h, w, bnn_out));
    const size_t nb = (size_t)bh * bw;
    HostCall hc(ctx);
    const uint32_t *db = hc.in(bnn_prev, nb), *dfw = hc.in(fwd, (size_t)h * w);
    uint32_t* dout = hc.out(bnn_out, nb);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_nnf_remap(ctx, ctx->stream, db, bh, bw, dfw, h, w, dout));
    return hc.finish();
}

int nct_nnf_merge(nct_ctx* ctx, const float* a_chw, const float* b_chw, int C, int ah, int aw, int bh, int bw, int patch, const uint32_t* z, const uint32_t* c,
                  uint32_t* start_out, float* dz_out, float* dc_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_nnf_merge_check(ctx, "nnf_merge", a_chw, b_chw, C, ah, aw, bh, bw, patch, z, c, start_out));
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    HostCall hc(ctx);
    float *t = hc.scratch<float>((size_t)C * (na > nb ? na : nb)), *A = hc.scratch<float>(C * na), *B = hc.scratch<float>(C * nb);
    uint32_t* ds = hc.inout(z, start_out, na);                   // Z goes up into the block the merge writes in place
    const uint32_t* dc = hc.in(c, na);
    float *ddz = hc.out(dz_out, na), *ddc = hc.out(dc_out, na);
    NCT_TRY(hc.ready());
    NCT_TRY(upload_hwc(ctx, hc, a_chw, t, A, C, (int)na));
    NCT_TRY(upload_hwc(ctx, hc, b_chw, t, B, C, (int)nb));
    NCT_TRY(nctk_nnf_merge(ctx, ctx->stream, A, B, nullptr, nullptr, C, ah, aw, bh, bw, NCT_PM_PLAIN, ds, dc, ddz, ddc, nullptr, nullptr, nullptr, nullptr));
    return hc.finish();
}

// SPEC §6.15 rule 1 on host arrays: the matte and the guide up, one k_region_snap launch out of place, the snapped matte down
int nct_region_snap(nct_ctx* ctx, const uint8_t* mask, const uint8_t* lab, int H, int W, const nct_region_snap_params* params, uint8_t* mask_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_snap_check(ctx, "region_snap", mask, lab, H, W, params, mask_out));
    const size_t N = (size_t)H * W;
    HostCall hc(ctx);
    const uint8_t *dm = hc.in(mask, N), *dl = hc.in(lab, N * 3);
    uint8_t* dout = hc.out(mask_out, N);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_region_snap(ctx, ctx->stream, dm, dl, H, W, params, dout));
    return hc.finish();
}

// SPEC §6.7 rule 1 on host maps: the two Lab level images (and the field) up, one k_seq_change launch, the 16-byte record down
int nct_seq_change(nct_ctx* ctx, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, const int16_t* field, int threshold, nct_seq_change_rec* out) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(lab && lab_prev, "seq_change: null image");
    NCT_REQUIRE(out, "seq_change: null out");
    NCT_REQUIRE(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seq_change: grid %dx%d out of range", w, h);
    NCT_REQUIRE(threshold >= 0 && threshold <= 765, "seq_change: the threshold must be in [0, 765] (got %d)", threshold);
    const size_t n = (size_t)h * w;
    HostCall hc(ctx);
    const uint8_t *dl = hc.in(lab, 3 * n), *dlp = hc.in(lab_prev, 3 * n);
    const int16_t* df = hc.in(field, 2 * n);
    nct_seq_change_rec* dr = hc.out(out, 1);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_seq_change(ctx, ctx->stream, dl, dlp, h, w, df, threshold, dr));
    return hc.finish();
}

int nct_bds_vote_image(nct_ctx* ctx, const uint8_t* a_bgr, int ah, int aw, const uint8_t* b_bgr, int bh, int bw,
                       const uint32_t* ann, const uint32_t* bnn, int patch, double w_coherence, double w_complete, uint8_t* out_bgr) {
    NCT_CTX_ENTER();
    (void)a_bgr;   // reconstruct_bds only uses a's size (GeneralizedPatchMatch.cu:124-131)
    NCT_REQUIRE(b_bgr && ann && bnn && out_bgr, "bds_vote_image: null pointer");
    NCT_REQUIRE(patch == 3, "bds_vote_image: only patch=3 is supported, got %d", patch);
    NCT_REQUIRE(ah > 0 && aw > 0 && bh > 0 && bw > 0, "bds_vote_image: empty image");
    NCT_REQUIRE(nct_nnf_dims_ok(ah, aw, bh, bw), "bds_vote_image: dims out of range (%dx%d vs %dx%d); NNF coordinates are 12-bit", ah, aw, bh, bw);
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    HostCall hc(ctx);
    const uint8_t* b = hc.in(b_bgr, nb * 3);
    uint8_t* o = hc.out(out_bgr, na * 3);
    const uint32_t *da = hc.in(ann, na), *db = hc.in(bnn, nb);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_bds_vote_image(ctx, ctx->stream, b, da, db, ah, aw, bh, bw, w_coherence, w_complete, o));
    return hc.finish();
}

// ---------------------------------------------------------------- measurement hooks
int nct_pm_bench_setup(nct_ctx* ctx, const float* a_chw, const float* b_chw, int C, int ah, int aw, int bh, int bw) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(a_chw && b_chw, "pm_bench_setup: null pointer");
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    if (ctx->bench_a) { (void)hipFree(ctx->bench_a); ctx->bench_a = nullptr; }
    if (ctx->bench_b) { (void)hipFree(ctx->bench_b); ctx->bench_b = nullptr; }
    if (ctx->bench_ah16) { (void)hipFree(ctx->bench_ah16); ctx->bench_ah16 = nullptr; }
    if (ctx->bench_bh16) { (void)hipFree(ctx->bench_bh16); ctx->bench_bh16 = nullptr; }
    NCT_HIP(hipMalloc(&ctx->bench_a, sizeof(float) * C * na));
    NCT_HIP(hipMalloc(&ctx->bench_b, sizeof(float) * C * nb));
    NCT_HIP(hipMalloc(&ctx->bench_ah16, 2 * (size_t)C * na));
    NCT_HIP(hipMalloc(&ctx->bench_bh16, 2 * (size_t)C * nb));
    if (!ctx->d_counter) NCT_HIP(hipMalloc(&ctx->d_counter, 32 * sizeof(unsigned long long)));
    {
        HostCall hc(ctx);
        float *t = hc.scratch<float>((size_t)C * (na > nb ? na : nb)), *x = hc.scratch<float>((size_t)C * (na > nb ? na : nb));
        NCT_TRY(hc.ready());
        NCT_TRY(upload_hwc(ctx, hc, a_chw, t, x, C, (int)na));
        NCT_TRY(nctk_normalize(ctx, ctx->stream, x, ctx->bench_a, nullptr, C, (int)na, ctx->bench_ah16));
        NCT_TRY(upload_hwc(ctx, hc, b_chw, t, x, C, (int)nb));
        NCT_TRY(nctk_normalize(ctx, ctx->stream, x, ctx->bench_b, nullptr, C, (int)nb, ctx->bench_bh16));
        NCT_TRY(hc.finish());
    }
    ctx->bench_C = C; ctx->bench_ah = ah; ctx->bench_aw = aw; ctx->bench_bh = bh; ctx->bench_bw = bw;
    return NCT_OK;
}

int nct_pm_bench_run(nct_ctx* ctx, int iters, int rs_max, uint32_t seed, float* kernel_ms, uint64_t* evals, uint32_t* nnf_out, float* dist_out) {
    NCT_CTX_ENTER();
    if (!ctx->bench_a) return ctx->fail(NCT_ERR_STATE, "pm_bench_run: call nct_pm_bench_setup first");
    const int C = ctx->bench_C, ah = ctx->bench_ah, aw = ctx->bench_aw, bh = ctx->bench_bh, bw = ctx->bench_bw;
    const size_t na = (size_t)ah * aw;
    DevBuf<uint32_t> n;
    DevBuf<float> d;
    if (!n.alloc(ctx, na) || !d.alloc(ctx, na)) return NCT_ERR_HIP;
    NCT_TRY(nctk_nnf_init(ctx, ctx->stream, n, ah, aw, bh, bw));
    unsigned long long* counter = evals ? ctx->d_counter : nullptr;
    if (counter) NCT_HIP(hipMemsetAsync(counter, 0, 4 * sizeof(unsigned long long), ctx->stream));
    NCT_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    NCT_TRY(nctk_patchmatch(ctx, ctx->stream, ctx->bench_a, ctx->bench_b, C, ah, aw, bh, bw, iters, rs_max, seed, n, d, counter));
    NCT_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    NCT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    NCT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (kernel_ms) *kernel_ms = ms;
    if (evals) { unsigned long long h = 0; NCT_HIP(hipMemcpy(&h, counter, sizeof h, hipMemcpyDeviceToHost)); *evals = (uint64_t)h; }
    if (nnf_out) NCT_HIP(hipMemcpy(nnf_out, n, sizeof(uint32_t) * na, hipMemcpyDeviceToHost));
    if (dist_out) NCT_HIP(hipMemcpy(dist_out, d, sizeof(float) * na, hipMemcpyDeviceToHost));
    return NCT_OK;
}

int nct_pm_bench_run_bidir(nct_ctx* ctx, int iters, int rs_max, uint32_t seed, int pm_mode, float* kernel_ms, uint64_t* counters, uint32_t* ann_out, float* annd_out,
                           uint32_t* bnn_out, float* bnnd_out) {
    NCT_CTX_ENTER();
    if (!ctx->bench_a) return ctx->fail(NCT_ERR_STATE, "pm_bench_run_bidir: call nct_pm_bench_setup first");
    NCT_REQUIRE(pm_mode >= NCT_PM_PLAIN && pm_mode <= NCT_PM_FP16, "pm_bench_run_bidir: pm_mode must be 0 (fp32), 1 (fp32 + row rejection) or 2 (fp16)");
    const int C = ctx->bench_C, ah = ctx->bench_ah, aw = ctx->bench_aw, bh = ctx->bench_bh, bw = ctx->bench_bw;
    const size_t na = (size_t)ah * aw, nb = (size_t)bh * bw;
    DevBuf<uint32_t> an, bn;
    DevBuf<float> ad, bd;
    if (!an.alloc(ctx, na) || !bn.alloc(ctx, nb) || !ad.alloc(ctx, na) || !bd.alloc(ctx, nb)) return NCT_ERR_HIP;
    NCT_TRY(nctk_nnf_init(ctx, ctx->stream, an, ah, aw, bh, bw));
    NCT_TRY(nctk_nnf_init(ctx, ctx->stream, bn, bh, bw, ah, aw));
    unsigned long long* counter = counters ? ctx->d_counter : nullptr;
    if (counter) NCT_HIP(hipMemsetAsync(counter, 0, 4 * sizeof(unsigned long long), ctx->stream));
    NCT_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    NCT_TRY(nctk_patchmatch_bidir(ctx, ctx->stream, ctx->bench_a, ctx->bench_b, ctx->bench_ah16, ctx->bench_bh16, C, ah, aw, bh, bw, iters, rs_max, seed, seed ^ 0x5bd1e995u,
                             an, ad, bn, bd, pm_mode, counter));
    NCT_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    NCT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    NCT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (kernel_ms) *kernel_ms = ms;
    if (counters) { unsigned long long h[2] = {0, 0}; NCT_HIP(hipMemcpy(h, counter, sizeof h, hipMemcpyDeviceToHost)); for (int i = 0; i < 2; ++i) counters[i] = (uint64_t)h[i]; }
    if (ann_out) NCT_HIP(hipMemcpy(ann_out, an, sizeof(uint32_t) * na, hipMemcpyDeviceToHost));
    if (annd_out) NCT_HIP(hipMemcpy(annd_out, ad, sizeof(float) * na, hipMemcpyDeviceToHost));
    if (bnn_out) NCT_HIP(hipMemcpy(bnn_out, bn, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost));
    if (bnnd_out) NCT_HIP(hipMemcpy(bnnd_out, bd, sizeof(float) * nb, hipMemcpyDeviceToHost));
    return NCT_OK;
}

}  // extern "C"
