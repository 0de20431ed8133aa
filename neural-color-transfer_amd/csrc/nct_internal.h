// nct_internal.h — context, device-memory arena and launch helpers shared by the libnct translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cmath>
#include <deque>
#include <string>
#include <vector>
#include "../../include/nct.h"

struct nct_block { void* p; size_t bytes; bool used; };

struct nct_ctx {
    int device = 0;
    hipStream_t stream = nullptr;     // main stream (S->R direction, VGG, colour stage)
    hipStream_t stream2 = nullptr;    // side stream: the kNN graphs and S1 graph parts of a pair's levels, built beside the main stream's correspondence work (nct_pipeline.cpp)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr;
    hipEvent_t ev_level[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // side-stream completion of level l's kNN graph
    hipStream_t stream_wls = nullptr;  // helper stream of the split WLS solve (NCT_FLAG_LATENCY)
    hipEvent_t ev_wls_fork = nullptr, ev_wls_join = nullptr;
    void* pinned = nullptr;                        // 4 KB of page-locked host memory the WLS solver publishes its state to (k_wls_mg.hip: two slots per half-solve; + 64 B: s1_hub_blocks)
    std::string err;
    std::vector<nct_block> blocks;    // cached device allocations, reused across calls and pairs
    size_t bytes_allocated = 0;
    int arena_fill = -1;              // test hook (env NCT_ARENA_FILL=0..255): alloc() fills the whole block it hands out with this byte; -1 = off
    // measurement fixture (nct_pm_bench_*)
    float *bench_a = nullptr, *bench_b = nullptr; void *bench_ah16 = nullptr, *bench_bh16 = nullptr; int bench_C = 0, bench_ah = 0, bench_aw = 0, bench_bh = 0, bench_bw = 0;
    // opaque sub-states owned by other translation units
    void* vgg = nullptr;              // struct vgg_weights* (nct_vgg.cpp)
    void* cvt = nullptr;              // struct cvt_dev* (k_cvt.hip): colour-conversion LUTs on the device
    void* pair = nullptr;             // struct pair_state* (nct_pipeline.h): device-resident source/reference/result images
    void* lut_accum = nullptr;        // struct lut_accum* (nct_lut.cpp): the shot accumulator between nct_lut_accum_begin and _end (SPEC §6.20)
    void* reflib = nullptr;           // struct reflib_dev* (nct_reflib.cpp): the device copy of the library nct_reflib_rank last ranked against (SPEC §6.21)
    unsigned long long* d_counter = nullptr;   // device counters of the pm kernels (NCT_FLAG_COUNT_EVALS): [0] distance evaluations performed, [1] accepted candidates;
                                                // 4 slots per pyramid level in pair runs (nct_pipeline.cpp reads [4 l] and [4 l + 1])
    int home_xcd = 0;                           // the XCD this context's single-XCD launches aim at (k_s1.hip: small S1 levels); contexts of a process count round-robin (nct_create)
    unsigned pm_attr_mask = 0;                 // k_pm_step instantiations whose dynamic-LDS opt-in has been set on this context's device
    // stage clock: events recorded on the main stream at stage boundaries, read once after the pair's final synchronise
    // (no host syncs in between: see nct_pair_timing in nct.h)
    int wls_split = 0;                          // NCT_FLAG_LATENCY of the running pair: a- and b-half of the WLS solve on two streams
    int wls_forecast = 1;                       // size the PCG iteration batches by the host's convergence forecast (k_wls_mg.hip: pcg_part); NCT_WLS_FORECAST=0: fixed batches
    int wls_lines = 1;                          // block step of alternating line solves on the finest S2 level (k_wls_mg.hip: k_mg_block; oracle: mg_block_step). NCT_S2_LINES=0: the cycle without it (other arithmetic; comparison only)
    int conv_pool_fuse = -1;                    // VGG: 2x2 max-pool inside the conv epilogue: -1 = where the tile shape fits the map (nctk_conv3x3_pool_fits), 0 never, 1 always (NCT_CONV_POOL_FUSE; tests)
    double wls_rtol = 3e-8;                     // relative residual at which the WLS solve stops. The loosest tolerance at which the 8-bit result of every level equals the EXACT solve's on the
                                                // 700x700, mixed and 1000x1000 fixtures: 1e-7 with the point smoother of rounds 3-5a (1e-6: 55.4 / 50.1 dB), 3e-8 with the block step (the same residual norm
                                                // leaves more low-frequency error: 5e-8 differs in 53 bytes on the mixed pair; profiles/round5_wls_rtol_sweep.json). Experiment hook: env NCT_WLS_RTOL
    int wls_maxit = 5000;                       // iteration budget of the WLS solve (test hook: env NCT_WLS_MAXIT)
    bool wls_trace = false;                     // env NCT_WLS_TRACE: every (half-)solve prints the iterations it enqueued and needed and the snapshots it read (k_wls_mg.hip: pcg_part)
    int s1_maxit = 0;                           // S1 iteration cap; 0 = the reference's (50 at layer 4, else 100). Test hook: env NCT_S1_MAXIT
    bool tm_on = false;
    int tm_level = 0;                           // pyramid level whose colour stage is being enqueued: the level of the marks k_colorsolve.hip sets
    std::vector<hipEvent_t> tm_events;          // pool, reused across pairs
    std::vector<double> tm_host;                // host clock (us) at mark i: NCT_HOST_TRACE=1 prints it beside the GPU clock (how far the host runs ahead)
    std::vector<int> tm_tags;                   // tag of mark i = the stage that ENDS at event i
    int mark(hipStream_t s, int tag);           // nct_api.cpp; no-op unless tm_on
    // kernel clock (NCT_FLAG_TIME_KERNELS): event pairs around single launches of the full-resolution colour-solver kernels; sample i = events 2i, 2i+1, id kt_ids[i]
    int conv_pair = 1;                          // conv5_1 of the source and the reference in one launch (k_vgg.hip: nctk_conv3x3_pair); NCT_CONV_PAIR=0: two launches
    int* s1_hub_blocks() { return (int*)((char*)pinned + 4096); }   // [5][2] hub block and super-block count of each pyramid level's kNN graph (k_s1.hip), written by the side stream behind the WLS solver's 4 KB
    long long s1_hub_blocks_last[5] = {0, 0, 0, 0, 0};            // the counts the last pair's solves were launched with (-1: not known when the solve was enqueued); nct_ctx_counter
    int knn_runs = -1;                          // kNN search form: -1 = one search per (cluster, colour) run where runs average > 2.5 entries, decided on the device; 0 / 1 = NCT_KNN_RUNS (tests)
    int s1_hub_hint = 1;                        // use the host-side hub block counts (NCT_S1_HUB_HINT=0: always launch the hub pass — the conservative path, for tests)
    bool kt_on = false;
    std::vector<hipEvent_t> kt_events; std::vector<int> kt_ids;
    int kt_begin(hipStream_t s, int id);        // nct_api.cpp; no-ops unless kt_on
    int kt_end(hipStream_t s);

    double guided_sigma = 0.0;                  // nct_set_finish_guided (SPEC §6.10): > 0 = every upsampling finish behind a working-size finish runs guided with this sigma; 0 = off (the default)

    int fail(int code, const char* fmt, ...) {
        char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        err = buf; return code;
    }
    void* alloc(size_t bytes);        // never returns null on success; sets err and returns null on failure
    void release(void* p);
    // Arena blocks are recycled in stream order, which is only safe on ONE stream. While work is being enqueued on the side
    // stream, set defer_release: blocks released meanwhile stay reserved until flush_deferred() is called after the main
    // stream has been made to wait on the side stream's completion event.
    bool defer_release = false;
    std::vector<void*> deferred;
    void flush_deferred() { for (void* p : deferred) for (auto& b : blocks) if (b.p == p) { b.used = false; break; } deferred.clear(); }
};

// stage tags of the event marks (nct_ctx::mark): tag = stage * 8 + level; a mark closes the stage it names
enum { NCT_ST_OTHER = 0, NCT_ST_VGG, NCT_ST_CLUSTER, NCT_ST_PM, NCT_ST_VOTE, NCT_ST_KNN, NCT_ST_COLOR, NCT_ST_NONLOCAL, NCT_ST_WLS };
static inline int nct_stage_tag(int stage, int level) { return stage * 8 + level; }

// The one owner of a block from the context arena, scratch of a call or a member of long-lived state: allocated by its constructor, or empty (a member, an array
// element) until alloc(). The block goes back when the owner ends, or at reset()
template <typename T> struct DevBuf {
    nct_ctx* c = nullptr; T* p = nullptr;
    DevBuf() = default;
    DevBuf(nct_ctx* ctx, size_t n) { alloc(ctx, n); }
    ~DevBuf() { reset(); }
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    bool alloc(nct_ctx* ctx, size_t n) { reset(); c = ctx; p = (T*)ctx->alloc(n * sizeof(T)); return p != nullptr; }
    bool reserve(nct_ctx* ctx, size_t n) { return p || alloc(ctx, n); }      // a block that is reserved once and then kept: nothing is requested while the owner holds one
    void reset() { if (p) { c->release(p); p = nullptr; } }
    void swap(DevBuf& o) { nct_ctx* oc = o.c; T* op = o.p; o.c = c; o.p = p; c = oc; p = op; }
    void take(DevBuf& o) { reset(); c = o.c; p = o.p; o.p = nullptr; }        // o's block changes owner (what this one held goes back); o is left empty
    operator T*() const { return p; }
    bool ok() const { return p != nullptr; }
};

#define NCT_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return ctx->fail(NCT_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define NCT_LAUNCH_CHECK() NCT_HIP(hipGetLastError())
#define NCT_REQUIRE(cond, ...) do { if (!(cond)) return ctx->fail(NCT_ERR_INVALID, __VA_ARGS__); } while (0)
// an int-returning call (nctk_*, nct_ctx::mark, …) whose failure ends the calling function with the same code
#define NCT_TRY(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)
// what the C-ABI entry points open and move data with: a null context is refused, the context's device is made current; copies and the wait are on the main stream
#define NCT_CTX_ENTER() do { if (!ctx) return NCT_ERR_INVALID; NCT_HIP(hipSetDevice(ctx->device)); } while (0)
#define NCT_H2D(dst, src, bytes) NCT_HIP(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, ctx->stream))
#define NCT_D2H(dst, src, bytes) NCT_HIP(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, ctx->stream))
#define NCT_SYNC() NCT_HIP(hipStreamSynchronize(ctx->stream))

// One host-pointer entry point's traffic on the main stream: the call's arena blocks, its uploads (enqueued at once) and its downloads (enqueued by finish(), in the
// order they were asked for, in front of the call's one wait). The first failed reservation or copy sticks: what follows it does nothing and returns null, and the
// entry point tests ready() once before its first launcher. The blocks are DevBufs: they go back when the call ends — behind the wait where it succeeds; where it fails
// after a copy was enqueued the destructor waits first (its own error is dropped: the call has its code and message), so that no call returns while a copy from or
// to the caller's memory is still queued
struct HostCall {
    nct_ctx* ctx; int rc = NCT_OK; bool queued = false, waited = false;
    struct Down { void* host; const void* dev; size_t bytes; };
    std::vector<Down> downs;
    std::deque<DevBuf<char>> blocks;
    explicit HostCall(nct_ctx* c) : ctx(c) {}
    HostCall(const HostCall&) = delete; HostCall& operator=(const HostCall&) = delete;
    ~HostCall() { if (queued && !waited) (void)hipStreamSynchronize(ctx->stream); }
    template <typename T> T* scratch(size_t n) {                                  // a block of n elements that nobody copies
        if (rc) return nullptr;
        blocks.emplace_back();
        if (!blocks.back().alloc(ctx, n * sizeof(T))) rc = NCT_ERR_HIP;
        return (T*)blocks.back().p;
    }
    // the copies alone, for a block that holds several arrays or is used twice (a null side: nothing)
    template <typename T> void put(T* dev, const T* host, size_t n) { if (!rc && dev && host) copy(dev, host, n * sizeof(T), hipMemcpyHostToDevice); }
    template <typename T> void get(T* host, const T* dev, size_t n) { if (!rc && dev && host) downs.push_back({host, dev, n * sizeof(T)}); }
    // an argument of the call: a null host array reserves nothing and gives the launcher null
    template <typename T> T* in(const T* host, size_t n) { return inout(host, (T*)nullptr, n); }
    template <typename T> T* out(T* host, size_t n) { return inout((const T*)nullptr, host, n); }
    template <typename T> T* inout(const T* src, T* dst, size_t n) {              // up now, down at finish(): a seam that runs in place
        if (!src && !dst) return nullptr;
        T* d = scratch<T>(n);
        put(d, src, n); get(dst, d, n);
        return rc ? nullptr : d;
    }
    int ready() const { return rc; }                                              // the first failure so far (its message is in ctx->err), else NCT_OK
    int finish() {
        for (size_t i = 0; i < downs.size() && !rc; ++i) copy(downs[i].host, downs[i].dev, downs[i].bytes, hipMemcpyDeviceToHost);
        if (rc) return rc;
        waited = true;
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        return e == hipSuccess ? NCT_OK : (rc = ctx->fail(NCT_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e)));
    }
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        queued = true;
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
        if (e != hipSuccess) rc = ctx->fail(NCT_ERR_HIP, "hipMemcpyAsync (%s, %zu bytes) failed: %s", kind == hipMemcpyHostToDevice ? "host to device" : "device to host", bytes, hipGetErrorString(e));
    }
};

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// the largest element count (C * H * W, H * W) a launcher takes as an int: cdiv rounds it up by at most 255 without leaving the type
#define NCT_MAX_ELEMS (2147483647LL - 255)
// the four dimensions of a field between two maps: the NNF word holds 12 bits per coordinate
static inline bool nct_nnf_dims_ok(int ah, int aw, int bh, int bw) { return ah >= 1 && aw >= 1 && bh >= 1 && bw >= 1 && ah < 4096 && aw < 4096 && bh < 4096 && bw < 4096; }
// host-side functions and types shared between translation units that stay out of the library's dynamic symbol table
#define NCT_LOCAL __attribute__((visibility("hidden")))
// a host copy for level-wise validation (host nullable): enqueued and waited for
template <typename T> static inline int dbg_copy(nct_ctx* ctx, hipStream_t s, T* host, const void* dev /* n elements of T */, size_t n) {
    if (!host) return 0;
    NCT_HIP(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, s));
    NCT_HIP(hipStreamSynchronize(s));
    return 0;
}

// ---- device-side launchers (all on device pointers, features channel-last HWC fp32) ----
// k_feat.hip
int nctk_chw_to_hwc(nct_ctx* ctx, hipStream_t s, const float* src, float* dst, int C, int HW);
int nctk_hwc_to_chw(nct_ctx* ctx, hipStream_t s, const float* src, float* dst, int C, int HW);
int nctk_normalize(nct_ctx* ctx, hipStream_t s, const float* src_hwc, float* dst_hwc, float* resp /*nullable*/, int C, int HW,
                   void* dst_h16 = nullptr /* nullable: fp16 (round-to-nearest) shadow copy of dst, same HWC layout */);
int nctk_feature_distance(nct_ctx* ctx, hipStream_t s, const float* a_hwc, const float* b_hwc, float* err, int C, int HW);
// k_nnf.hip
int nctk_nnf_init(nct_ctx* ctx, hipStream_t s, uint32_t* nnf, int ah, int aw, int bh, int bw);
int nctk_nnf_upsample(nct_ctx* ctx, hipStream_t s, const uint32_t* nnf_half, uint32_t* nnf, int ah, int aw, int bh, int bw, int ah_half, int aw_half);
// k_patchmatch.hip — nnf in/out, dist out; tmp buffers come from the arena
int nctk_patchmatch(nct_ctx* ctx, hipStream_t s, const float* a_hwc, const float* b_hwc, int C, int ah, int aw, int bh, int bw,
                    int iters, int rs_max, uint32_t seed, uint32_t* nnf, float* dist, unsigned long long* eval_counter /*nullable*/);
// k_vgg.hip / nct_vgg.cpp
// one conv layer: in = Cin (even: a zero pad plane for an odd layer) planar maps, wp = weights packed by nctk_pack_weights; out (planar; pool = 1: only the 2x2/2 pooled map) and
// out_hwc (channel-last, pool == 0 only) are each nullable, not both
int nctk_conv3x3(nct_ctx* ctx, hipStream_t s, const float* in, const float* wp, const float* bias, float* out, int Cin, int Cout, int H, int W, int relu, int pool, float* out_hwc = nullptr);
int nctk_pack_weights(nct_ctx* ctx, hipStream_t s, const float* w /*[Cout][Cin][3][3]*/, float* wp /*[Cin_pad*9][Cout]*/, int Cout, int Cin, int Cin_pad);
int nctk_conv3x3_pair(nct_ctx* ctx, hipStream_t s, const float* in1, int H1, int W1, const float* in2, int H2, int W2, const float* wp, const float* bias,
                      float* out1, float* out2, int Cin, int Cout, int relu, float* hwc1, float* hwc2);
// both images to conv5_1 (channel-last taps only), the last layer for both in one launch
int nctk_vgg19_forward_pair(nct_ctx* ctx, hipStream_t s, const uint8_t* d_bgr1, int H1, int W1, int stride1, float* const* taps_hwc1,
                            const uint8_t* d_bgr2, int H2, int W2, int stride2, float* const* taps_hwc2);
int nctk_vgg19_forward(nct_ctx* ctx, hipStream_t s, const uint8_t* d_bgr, int H, int W, int stride, int deepest_tap, float* const* d_taps_chw, int* dims,
                       float* const* d_taps_hwc = nullptr /* the same taps channel-last, written by the tap layers' epilogues */);
void nct_vgg_free(nct_ctx* ctx);
// k_cvt.hip
int nctk_bgr2lab(nct_ctx* ctx, hipStream_t s, const uint8_t* src, uint8_t* dst, size_t npix);
int nctk_lab2bgr(nct_ctx* ctx, hipStream_t s, const uint8_t* src, uint8_t* dst, size_t npix, int form = 0 /* 0 = piecewise form (default), 1 = plain-cube form: k_cvt.hip */);
int nctk_resize_u8c3(nct_ctx* ctx, hipStream_t s, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);
int nctk_resize_f64c3(nct_ctx* ctx, hipStream_t s, const double* src, int sh, int sw, double* dst, int dh, int dw);
int nctk_cvt_tables(nct_ctx* ctx, const void** tables);   // the context's conversion tables on the device (struct CvtTables, nct_pixel.h), built at first use
void nct_cvt_free(nct_ctx* ctx);
void nct_pair_free(nct_ctx* ctx);   // nct_pipeline.cpp
// k_cluster.hip
int nctk_kmeans_labels(nct_ctx* ctx, hipStream_t s, const float* feat_hwc_norm, int n, int C, int K, int iters, uint64_t seed, int* labels, int* nlabels_dev);
int nctk_knn_graph(nct_ctx* ctx, hipStream_t s, const uint8_t* lab_u8, int h, int w, const int* labels, int lh, int lw, int nlabels, const int* nlabels_dev /*nullable: overrides nlabels*/, int samples,
                   int* knn_id, double* knn_w);
// k_s1.hip — S1, the nonlocal truncated CG. The graph-only part of its system depends on the level's kNN graph alone and is built once per level (in the pipeline: on the
// side stream, right behind the graph); nseg_hint is what the HOST knows about the number of hub blocks when it enqueues the solve (-1: nothing, the hub pass is launched anyway)
#define NCT_S1_SEG 64                        // in-edges of a pixel summed one by one; every further block of this many is summed by a tree in the hub pass
struct nct_s1_graph {
    int n;
    double* iw2;                             // [n][8] squared nonlocal weight of every out-edge
    unsigned long long* starts;              // [n + 1] low half: start of the pixel's first block (<= 64 in-edges) in c_src / c_w; high half: index of its first hub block
    int* c_src; double* c_w;                 // compact arrays of the first blocks
    int* rev_start;                          // [n + 1] start of the pixel's in-edges in the target-sorted edge list
    int* rev_src; double* rev_w;             // that list by position (only entries behind a first block are written and read)
    int* seg_tgt; int* seg_e0;               // hub block table: target pixel, position of the block's first edge
    double* hub_part;                        // [blocks][6] block sums of the current operator pass
    int* sup_start;                          // [n + 1] index of the pixel's first SUPER-block (64 hub blocks; only pixels with more than 64 hub blocks have any); sup_start[n] = their number
    int* sup_b0;                             // [super-blocks] index of the super-block's first hub block (its last: min(b0 + 64, the pixel's last block))
    double* sup_part;                        // [super-blocks][6] super-block sums of the current operator pass
    int nseg_hint, nsup_hint;                // what the host knows about the two counts (-1: nothing yet)
};
struct nct_s1_graph_bufs {
    int n = 0;
    DevBuf<double> iw2, c_w, rev_w, hub_part, sup_part; DevBuf<unsigned long long> starts; DevBuf<int> c_src, rev_start, rev_src, seg_tgt, seg_e0, sup_start, sup_b0;
    bool alloc(nct_ctx* c, int n_) {
        n = n_;
        return iw2.alloc(c, (size_t)8 * n_) && c_w.alloc(c, (size_t)8 * n_) && rev_w.alloc(c, (size_t)8 * n_) && hub_part.alloc(c, ((size_t)n_ / 8 + 1) * 6) && sup_part.alloc(c, ((size_t)n_ / 256 + 2) * 6) &&
               starts.alloc(c, (size_t)n_ + 1) && c_src.alloc(c, (size_t)8 * n_) && rev_start.alloc(c, (size_t)n_ + 1) && rev_src.alloc(c, (size_t)8 * n_) && seg_tgt.alloc(c, (size_t)n_ / 8 + 1) &&
               seg_e0.alloc(c, (size_t)n_ / 8 + 1) && sup_start.alloc(c, (size_t)n_ + 1) && sup_b0.alloc(c, (size_t)n_ / 256 + 2);
    }
    nct_s1_graph view(int hint, int hint2) const { return nct_s1_graph{n, iw2, starts, c_src, c_w, rev_start, rev_src, rev_w, seg_tgt, seg_e0, hub_part, sup_start, sup_b0, sup_part, hint, hint2}; }
};
int nctk_s1_graph_build(nct_ctx* ctx, hipStream_t s, const int* knn_id, const double* knn_w, double nonlocalWeight, const nct_s1_graph& g, int* nseg_pinned /*nullable: [2] hub blocks, super-blocks*/);
int nctk_s1_solve(nct_ctx* ctx, hipStream_t s, const nct_s1_graph& g, const int* knn_id, const double* weight, float dWeight, const uint8_t* s_lab_level,
                  const uint8_t* g_lab_level, const double* gx, const double* gy, int layer, int h, int w, double* x, int* cg_iters_host);
// k_colorsolve.hip
struct nct_color_params { double eps, nonlocal_weight, local_weight, wls_lambda_init, wls_alpha, k_num; };
static inline nct_color_params nct_color_params_of(const nct_params& p) { return {p.eps, p.nonlocal_weight, p.local_weight, p.wls_lambda_init, p.wls_alpha, (double)p.k_num}; }
static inline int nct_cube_form(const nct_params& p) { return (p.flags & NCT_FLAG_LAB2BGR_CUBE) ? 1 : 0; }   // the Lab -> BGR form of nctk_lab2bgr
// the solvers' domain (include/nct.h at nct_params): T1 divides by eps, S1 takes roots of both weights, S2 of lambda, and nct_pow(., wls_alpha) is defined for an exponent
// > 0; the vote weighs with bds_weight. One rule for every entry point (`who`) that takes the struct: the first field outside it is named, before anything is enqueued
static inline int nct_params_check(nct_ctx* ctx, const char* who, const nct_params& p) {
    const struct { const char* name; double v; bool zero_ok; } fields[] = {{"bds_weight", p.bds_weight, true}, {"eps", p.eps, false}, {"nonlocal_weight", p.nonlocal_weight, false},
        {"local_weight", p.local_weight, false}, {"wls_lambda_init", p.wls_lambda_init, false}, {"wls_alpha", p.wls_alpha, false}};
    for (const auto& f : fields)
        if (!std::isfinite(f.v) || !(f.zero_ok ? f.v >= 0.0 : f.v > 0.0))
            return ctx->fail(NCT_ERR_INVALID, "%s: %s must be finite and %s (got %g)", who, f.name, f.zero_ok ? ">= 0" : "> 0", f.v);
    return NCT_OK;
}
struct nct_color_debug { double *ab_local, *ab_nonlocal, *ab_up, *rough, *ab_wls; int* cg_iters; int* wls_iters; };   // host pointers, all nullable
// the largest finish target: S2's hierarchy stays within MG_MAXL levels (nct_wls_plan.h) and each of its arrays below 4 GB (6 fp64 right-hand sides: 3.2 GB)
#define NCT_FINISH_MAX_SIDE 16384
#define NCT_FINISH_MAX_PIXELS (1LL << 26)
// the upsampling finish behind a working-size finish (SPEC §6.8): the original source in BGR at H x W, where its result goes, the Lab -> BGR form
// sigma > 0: the guided finish (SPEC §6.10) with the working-size Lab image of that finish as its guide; 0: the plain bilinear one
// mask (nullable): the masked upsampling finish (SPEC §6.13 rule 4) — the source's region mask at H x W and nct_region_params.protect
struct nct_finish_up { const uint8_t* s_bgr; int H, W; uint8_t* out_bgr; int form; double sigma; const uint8_t* mask; int protect; };
// what a level's colour stage keeps reserved from T1 until its finish has been enqueued, declared by the caller: the coefficients x ([2][h*w][3]: T1's guess, then S1's
// output), T2's weights and extremes and — requested between S1 and the finish by a frame of a sequence that reports it (SPEC §6.3) — the tau_p map
struct NCT_LOCAL nct_color_bufs { DevBuf<double> x, weight; DevBuf<unsigned> mm; DevBuf<double> tmap; };
// T1, T2 and S1 of a level: its coefficients into b.x. H x W: the working size (S1's dWeight); the finish (nctk_color_finish) reads b.x afterwards
NCT_LOCAL int nctk_color_nonlocal(nct_ctx* ctx, hipStream_t s, const float* err, const uint8_t* s_lab_level, const uint8_t* g_lab_level, const int* knn_id, const double* knn_w,
                                  int layer, int h, int w, int H, int W, const nct_color_params& prm, nct_color_bufs& b, const nct_color_debug* dbg,
                                  const nct_s1_graph* graph = nullptr /* the level's prebuilt graph part of S1; null: built inside, on s */);
// U1 + roughness + S2 + A1 of coefficients x ([2][h*w][3], device) onto the grid H x W of s_lab_full; Hw x Ww = the working size (the x4 of S2's lambda).
// up (nullable): S2's output, still on the device, then also goes through the upsampling finish onto up's source
int nctk_color_finish(nct_ctx* ctx, hipStream_t s, const double* x, int h, int w, int Hw, int Ww, const uint8_t* s_lab_full, int H, int W,
                      const nct_color_params& prm, uint8_t* out_lab_full, const nct_color_debug* dbg, const nct_finish_up* up = nullptr);
// k_finish_up.hip — the upsampling finish onto up's source, one kernel: ab_wls ([2][h*w][3], device) upsampled (U1's arithmetic; up.sigma > 0: SPEC §6.10's joint-bilateral
// weights, with lab_work ([h*w][3], device, else nullable), the 8-bit Lab image of the working-size source, as the guide) and applied (A1's) to up.s_bgr (up.H x up.W >=
// h x w), BGR in, BGR out; with up.mask the compose of SPEC §6.11 rule 3 rides in the place of the Lab -> BGR. Equal sizes: the plain pass's copy path in every form
int nctk_finish_up(nct_ctx* ctx, hipStream_t s, const double* ab_wls, const uint8_t* lab_work, int h, int w, const nct_finish_up& up);
// its checks, for a caller that has to refuse before it reserves or uploads anything. `guided` is the form the caller asked for: a guided entry point is refused for a
// sigma that nctk_finish_up would read as "plain". The messages name the form (nct_finish_up_name)
int nctk_finish_up_check(nct_ctx* ctx, bool guided, const void* ab_wls, const void* lab_work, int h, int w, const nct_finish_up& up);
static inline const char* nct_finish_up_name(bool guided, bool masked) {
    return guided ? (masked ? "color_finish_guided_region" : "color_finish_guided") : (masked ? "color_finish_upsample_region" : "color_finish_upsample");
}
// sigma and sigma^2 (what the kernel divides by) are finite and > 0
static inline bool nct_guided_sigma_ok(double sigma) { const double s2 = sigma * sigma; return sigma > 0.0 && s2 > 0.0 && s2 <= 1.7976931348623157e308; }
// SPEC §6.1 rule 1 + the limits of rule 5: nullptr and the working size, or the reason the image is refused (a static string)
const char* nct_working_size_rule(int h, int w, int max_side, int* work_h, int* work_w);
void nct_set_ctxless_error(const char* msg);   // nct_api.cpp
// k_select.hip — SPEC §6.2 rules 2-3: per pixel the reference with the smallest 3 x 3 error sum, and G / E merged by that label. err / guide: host arrays of K device
// pointers (they go into the kernel's argument block); label, guide_out (then guide may be null too) and err_out are nullable
int nctk_select_reference(nct_ctx* ctx, hipStream_t s, const float* const* err, const uint8_t* const* guide, int K, int h, int w,
                          uint8_t* label, uint8_t* guide_out, float* err_out);
// k_select_hold.hip — SPEC §6.18 rules 1-6: nctk_select_reference with a memory. prev_label ([h*w] bytes): the labels the previous frame kept, read at p + m(p);
// lab / lab_prev ([h*w][3] 8-bit Lab): the two frames' level images, for the gain g of nctk_seq_blend; field (nullable: m = 0) as there; hold in [0, 2], sigma > 0.
// label, guide_out (then guide may be null too), err_out, free_label (rule 1's f) and margin (rule 4's value, [h*w] doubles) are nullable; label must not overlap prev_label
int nctk_select_hold(nct_ctx* ctx, hipStream_t s, const float* const* err, const uint8_t* const* guide, int K, int h, int w, const uint8_t* prev_label, const uint8_t* lab,
                     const uint8_t* lab_prev, const int16_t* field, double hold, double sigma, uint8_t* label, uint8_t* guide_out, float* err_out, uint8_t* free_label,
                     double* margin);
// its argument checks (`who` names the entry point in the message), for the host form to run before it moves anything, and the range of hold alone
int nct_select_hold_check(nct_ctx* ctx, const char* who, const void* const* err, const void* const* guide, int K, int h, int w, const void* prev_label, const void* lab,
                          const void* lab_prev, double hold, double sigma, const void* guide_out);
bool nct_seq_hold_ok(double hold);
// SPEC §6.18 rule 7: label_out(p) = label_prev(p + m(p)), a vector that leaves the grid clamped to it; label_out must not overlap label_prev
int nctk_label_carry(nct_ctx* ctx, hipStream_t s, const uint8_t* label_prev, int h, int w, const int16_t* field, uint8_t* label_out);
// k_seq_pull.hip — SPEC §6.19 rules 2-4 in one launch: P_l = the pulled mask of the pixel's label (pulled: K device pointers, null = 255; label is read with K > 1
// only), P' = P_l held against prev ([h*w] bytes, the map the previous frame kept, read at p + m(p)) with nctk_seq_blend's weight tau_p on lab / lab_prev, M = min(P',
// src_mask) (null = 255). field (nullable: m = 0) as there. m_out and p_free (P_l before the hold) are nullable; p_out must not overlap prev
int nctk_seq_pull_hold(nct_ctx* ctx, hipStream_t s, const uint8_t* const* pulled, int K, const uint8_t* label, const uint8_t* prev, const uint8_t* lab, const uint8_t* lab_prev,
                       const int16_t* field, const uint8_t* src_mask, int h, int w, double tau, double sigma, uint8_t* p_out, uint8_t* m_out, uint8_t* p_free);
// its argument checks (`who` names the entry point in the message), for the host form to run before it moves anything
int nct_seq_pull_hold_check(nct_ctx* ctx, const char* who, const void* const* pulled, int K, const void* label, const void* prev, const void* lab, const void* lab_prev, int h, int w,
                            double tau, double sigma, const void* p_out);
// k_temporal.hip — SPEC §6.3 rule 3: x_out = x + tau_p (x_prev - x) per level pixel, tau_p from the 3 x 3 mean squared Lab difference; x_out may alias x or x_prev; tau_map nullable.
// field (nullable, [h*w][2] int16 (my, mx)): SPEC §6.4 rule 4 — L_(t-1) and x_prev are read at p + m(p); x_out may then alias x only
int nctk_seq_blend(nct_ctx* ctx, hipStream_t s, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                   double* x_out, double* tau_map, const int16_t* field = nullptr);
// the argument checks of nct_seq_blend and nct_seq_blend_mc (one message for both: a blend without a field is the first), in front of their reservations
int nct_seq_blend_check(nct_ctx* ctx, const void* x, const void* x_prev, const void* lab, const void* lab_prev, int h, int w, const void* x_out, const void* field);
// SPEC §6.4 rules 1-3: the level's motion field from L_t ([n][3] bytes) and L_(t-1) packed by nctk_seq_pack ([n] words L | a << 8 | b << 16); parent nullable
int nctk_seq_pack(nct_ctx* ctx, hipStream_t s, const uint8_t* lab, int n, uint32_t* out);
int nctk_seq_motion(nct_ctx* ctx, hipStream_t s, const uint8_t* lab, const uint32_t* prev_packed, int h, int w, const int16_t* parent, int ph, int pw, int R, int penalty,
                    int16_t* m_out);
// the argument checks of nct_seq_motion_field[_dev] (`who` names the entry point in the message), in front of the block of the packed image
int nct_seq_motion_field_check(nct_ctx* ctx, const char* who, const void* lab, const void* lab_prev, int h, int w, const void* parent, int ph, int pw, const void* m_out);
// SPEC §6.5 rule 3: x_out(p) = x_prev(p + m(p)), the 64-bit words copied, a vector that leaves the grid clamped to it; x_out must not overlap x_prev
int nctk_seq_warp(nct_ctx* ctx, hipStream_t s, const double* x_prev, int h, int w, const int16_t* field, double* x_out);
// SPEC §6.7 rule 1: sad = sum_p r(p), changed = #{p : r(p) > threshold}, pixels = h * w, r(p) the three-byte SAD of lab(p) and lab_prev(p + m(p)); field nullable (m = 0).
// rec: 16 bytes on the device, zeroed and filled on s
int nctk_seq_change(nct_ctx* ctx, hipStream_t s, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, const int16_t* field, int threshold, nct_seq_change_rec* rec);
// k_seq_track.hip — SPEC §6.14 rule 1: mask_out(p) = mask_prev(p + d(p)), d the field ([h*w][2] int16 (my, mx) on a level grid h x w <= H x W) interpolated at p, scaled to
// target pixels and rounded half up in integers, a position that leaves the matte clamped to it; mask_out must not overlap mask_prev
int nctk_seq_matte_warp(nct_ctx* ctx, hipStream_t s, const uint8_t* mask_prev, int H, int W, const int16_t* field, int h, int w, uint8_t* mask_out);
// its argument checks (`who` names the entry point in the message), for the host form to run before it moves anything
int nct_seq_matte_warp_check(nct_ctx* ctx, const char* who, const void* mask_prev, int H, int W, const void* field, int h, int w, const void* mask_out);
// k_seq_carry.hip — correspondence carry (SPEC §6.23). nctk_nnf_carry: rule 3, nnf_out(p) = nnf_prev(p + m(p)) on 32-bit words, the vector clamped component-wise;
// nnf_out must not overlap nnf_prev. nctk_nnf_forward_map: rule 4's F ([h*w] words (y << 12) | x) of a backward field — a fill, the minimum pass, the hole pass.
// nctk_nnf_remap: rule 4, bnn_out(q) = fwd(bnn_prev(q)) on the grid bh x bw, the word's coordinates clamped to fwd's grid h x w; bnn_out overlaps neither input.
// nctk_nnf_merge: rule 6 on normalised HWC maps — ann (and bnn; null: one direction, evaluated as nct_patchmatch does) hold Z and receive start, ca / cb are the moved
// kept fields, d* (nullable: scratch) receive the step-0 distances of Z and C. pm_mode and the fp16 shadows are nctk_patchmatch_bidir's
int nctk_nnf_carry(nct_ctx* ctx, hipStream_t s, const uint32_t* nnf_prev, int h, int w, const int16_t* field, uint32_t* nnf_out);
int nctk_nnf_forward_map(nct_ctx* ctx, hipStream_t s, const int16_t* field, int h, int w, uint32_t* fwd_out);
int nctk_nnf_remap(nct_ctx* ctx, hipStream_t s, const uint32_t* bnn_prev, int bh, int bw, const uint32_t* fwd, int h, int w, uint32_t* bnn_out);
int nctk_nnf_merge(nct_ctx* ctx, hipStream_t s, const float* a_hwc, const float* b_hwc, const void* a_h16, const void* b_h16, int C, int ah, int aw, int bh, int bw, int pm_mode,
                   uint32_t* ann, const uint32_t* ca, float* dza, float* dca, uint32_t* bnn, const uint32_t* cb, float* dzb, float* dcb);
// their argument checks (`who` names the entry point in the message), for the host forms to run before they move anything
int nct_nnf_carry_check(nct_ctx* ctx, const char* who, const void* nnf_prev, int h, int w, const void* field, const void* nnf_out);
int nct_nnf_forward_map_check(nct_ctx* ctx, const char* who, const void* field, int h, int w, const void* fwd_out);
int nct_nnf_remap_check(nct_ctx* ctx, const char* who, const void* bnn_prev, int bh, int bw, const void* fwd, int h, int w, const void* bnn_out);
int nct_nnf_merge_check(nct_ctx* ctx, const char* who, const void* a, const void* b, int C, int ah, int aw, int bh, int bw, int patch, const void* z, const void* c,
                        const void* start_out);
// k_region_snap.hip — SPEC §6.15 rule 1: mask_out(p) = the mean of mask over p's (2 radius + 1)^2 window inside the image, weighted with max(0, 3 sigma^2 - |lab(p) - lab(q)|^2)
// and rounded half up (binary: cut at 128 to 0 / 255); lab: the frame's 8-bit Lab image [H*W][3]; params null: the defaults; mask_out must overlap neither input
int nctk_region_snap(nct_ctx* ctx, hipStream_t s, const uint8_t* mask, const uint8_t* lab, int H, int W, const nct_region_snap_params* params, uint8_t* mask_out);
// its argument checks (`who` names the entry point in the message), for the host form to run before it moves anything, and the parameters' alone (null: the defaults)
int nct_region_snap_check(nct_ctx* ctx, const char* who, const void* mask, const void* lab, int H, int W, const nct_region_snap_params* params, const void* mask_out);
int nct_region_snap_params_check(nct_ctx* ctx, const char* who, const nct_region_snap_params* params);
// k_region_select.hip — region selection from strokes (SPEC §6.16). nctk_feat_quantize: rule 2 from the raw HWC tap, N1 (nctk_normalize's bits) and the int16 rows [HW][C].
// nctk_sel_cells: rule 3's cell flags (bit 0: an IN pixel, bit 1: an OUT pixel; [cells] words, zeroed here) and their exclusive scan pre [cells + 1] — low half the inside
// seed cells in front of the cell, high half the outside ones, the last word both totals. nctk_sel_seeds: with those totals n_* and the kept counts k_* = min(n_*,
// max_seeds): the cell codes of nct_region_select_stages.cell, the kept seeds' cells idx [k_in + k_out] (inside first) and their rows of q, seeds [k_in + k_out][C].
// nctk_region_score: rule 4 — code (nullable): the seed-cell overwrite by those codes. nctk_sel_stamp: rule 6's stamp in place
int nctk_feat_quantize(nct_ctx* ctx, hipStream_t s, const float* src_hwc, int16_t* dst, int C, int HW);
// the argument checks of nct_feat_quantize[_dev] (`who` names the entry point in the message, src_name / dst_name its two arrays, which the two forms call differently)
int nct_feat_quantize_check(nct_ctx* ctx, const char* who, const void* src, const char* src_name, const void* dst, const char* dst_name, int C, int H, int W);
int nctk_sel_cells(nct_ctx* ctx, hipStream_t s, const uint8_t* strokes, int h, int w, int tap, unsigned* flags, unsigned long long* pre);
int nctk_sel_seeds(nct_ctx* ctx, hipStream_t s, const int16_t* q, const unsigned* flags, const unsigned long long* pre, int cells, int C, unsigned n_in, unsigned n_out,
                   unsigned k_in, unsigned k_out, uint8_t* code, int* idx, int16_t* seeds);
int nctk_region_score(nct_ctx* ctx, hipStream_t s, const int16_t* q, int cells, int C, const int16_t* seeds_in, int n_in, const int16_t* seeds_out, int n_out, int sharpness,
                      int floor_permille, const uint8_t* code, uint8_t* score_out);
// its argument checks (`who` names the entry point in the message), for the host form to run before it moves anything
int nct_region_score_check(nct_ctx* ctx, const char* who, const void* q, int cells, int C, const void* seeds_in, int n_in, const void* seeds_out, int n_out, int sharpness,
                           int floor_permille, const void* score_out);
int nctk_sel_stamp(nct_ctx* ctx, hipStream_t s, const uint8_t* strokes, size_t n, uint8_t* m);
// k_region_refind.hip — SPEC §6.17 rules R1-R3 in one pass: out(p) = r(p) = nct_resize_u8c1(score: ht x wt -> H x W)(p) where prior is null or r(p) >= 128 + margin or
// r(p) < 128 - margin, else prior(p) (H x W bytes); H >= ht, W >= wt; out must overlap neither input
int nctk_region_refind(nct_ctx* ctx, hipStream_t s, const uint8_t* score, int ht, int wt, const uint8_t* prior, int H, int W, int margin, uint8_t* out);
// its argument checks (`who` names the entry point in the message), for the host form to run before it moves anything
int nct_region_refind_check(nct_ctx* ctx, const char* who, const void* score, int ht, int wt, int H, int W, int margin, const void* out);
// k_reflib.hip — reference libraries (SPEC §6.21). nctk_feat_quantize8: rule D2 from the raw HWC tap, center ([C] on the device) nullable, int8 rows [HW][C].
// nctk_descriptor_match: rule D3 — a [na][C], rows (the entries end to end), offsets ([N + 1] on the device; total = offsets[N], which the host knows), fwd / bwd [N]
// int64; its two transients come from the arena. The limits are the callers' (nct_reflib_host.h: reflib_table_check)
int nctk_feat_quantize8(nct_ctx* ctx, hipStream_t s, const float* src_hwc, const float* center, int8_t* dst, int C, int HW);
int nctk_descriptor_match(nct_ctx* ctx, hipStream_t s, const int8_t* a, int na, int C, const int8_t* rows, const int* offsets, int N, int total, long long* fwd, long long* bwd);
void nct_reflib_ctx_free(nct_ctx* ctx);   // nct_reflib.cpp
// k_lut.hip — 3D colour look-up tables (SPEC §6.6). W [N^3] / R [N^3][3]: the splat's integer sums (zeroed on s by the splat itself); D [N^3][3]: the displacement
// field after NCT_LUT_CYCLES V(2,2) cycles; lut [N^3][3] fp32. in / out of the apply may be the same buffer
#define NCT_LUT_CYCLES 17
#define NCT_LUT_MAX_PIXELS (1L << 26)
bool nct_lut_size_ok(int N);
// accumulate (SPEC §6.20, the shot accumulator): the splat adds to what W and R (and kept) hold — nothing is zeroed; nctk_lut_accum_zero is that zeroing alone (kept nullable)
int nctk_lut_accum_zero(nct_ctx* ctx, hipStream_t s, int N, uint64_t* W, int64_t* R, uint64_t* kept);
int nctk_lut_splat(nct_ctx* ctx, hipStream_t s, const uint8_t* src, const uint8_t* res, long npix, int N, uint64_t* W, int64_t* R, bool accumulate = false);
int nctk_lut_solve(nct_ctx* ctx, hipStream_t s, const uint64_t* W, const int64_t* R, int N, double lambda, double* D);
int nctk_lut_table(nct_ctx* ctx, hipStream_t s, const double* D, int N, float* lut);
int nctk_lut_apply(nct_ctx* ctx, hipStream_t s, const float* lut, int N, const uint8_t* in, long npix, uint8_t* out);
// SPEC §6.20: the table on 16-bit pixels ([npix][3] uint16, a value v standing for the grey level v / 257); in / out may be the same buffer
int nctk_lut_apply16(nct_ctx* ctx, hipStream_t s, const float* lut, int N, const uint16_t* in, long npix, uint16_t* out);
// the shot accumulator's cap on the pixels offered between begin and end: R stays below 2^62, W below 2^54 (SPEC §6.20)
#define NCT_LUT_ACCUM_MAX_PIXELS (1ULL << 30)
void nct_lut_accum_free(nct_ctx* ctx);   // nct_lut.cpp
// nct_pipeline.cpp — the images nct_pair_fit_lut reads after the context's last finished run (SPEC §6.6 rule 10), on the device; mask (null: every pixel) at their size.
// false: no finished run
struct nct_lut_images { const uint8_t *src, *res, *mask; size_t npix; int h, w; };
bool nct_pair_lut_images(nct_ctx* ctx, nct_lut_images* im);
// k_grid.hip — local colour grids (SPEC §6.22). sums / blurred [gy*gx*gz][22] int64 (sums zeroed on s by the splat itself); X [gy*gx*gz][3][4] double. in / out of an
// apply may be the same buffer
#define NCT_GRID_MAX_SIDE 16384
int nctk_grid_splat(nct_ctx* ctx, hipStream_t s, const uint8_t* src, const uint8_t* res, int H, int W, int gy, int gx, int gz, int64_t* sums);
int nctk_grid_solve(nct_ctx* ctx, hipStream_t s, const int64_t* sums, int gy, int gx, int gz, double lambda, int64_t* blurred, double* X);
int nctk_grid_apply(nct_ctx* ctx, hipStream_t s, const double* X, int gy, int gx, int gz, const uint8_t* in, int H, int W, uint8_t* out);
int nctk_grid_apply16(nct_ctx* ctx, hipStream_t s, const double* X, int gy, int gx, int gz, const uint16_t* in, int H, int W, uint16_t* out);
// nct_grid.cpp: the checks of nct_grid_fit's arguments (`what` names the entry point in the message), and splat + solve on device pointers, enqueued on the main
// stream; stages (nullable, its arrays nullable): DEVICE pointers
int nct_grid_fit_check(nct_ctx* ctx, const char* what, const void* src, const void* res, int h, int w, const nct_grid_params* prm, const void* grid_out);
int nct_grid_fit_enqueue(nct_ctx* ctx, const uint8_t* d_src, const uint8_t* d_res, int h, int w, const nct_grid_params* prm, double* d_grid, const nct_grid_stages* d_stages);
// nct_lut.cpp: the checks of nct_lut_fit's arguments (`what` names the entry point in the message), and splat + solve + table on device pointers, enqueued on the
// main stream; stages (nullable, its arrays nullable): DEVICE pointers
int nct_lut_fit_check(nct_ctx* ctx, const char* what, const void* src, const void* res, size_t npix, const nct_lut_params* prm, const void* lut_out);
int nct_lut_fit_enqueue(nct_ctx* ctx, const uint8_t* d_src, const uint8_t* d_res, size_t npix, const nct_lut_params* prm, float* d_lut, const nct_lut_stages* d_stages);
// SPEC §6.11 rule 7: the splat over the pixels with mask >= 128; kept (8 bytes on the device, zeroed on s): how many there were. nct_lut_fit_enqueue_masked: the fit with
// that splat (d_mask non-null); it waits for the splat to learn whether any pixel was kept and refuses an empty fit with NCT_ERR_INVALID (`what` names the entry point)
int nctk_lut_splat_masked(nct_ctx* ctx, hipStream_t s, const uint8_t* src, const uint8_t* res, const uint8_t* mask, long npix, int N, uint64_t* W, int64_t* R, uint64_t* kept,
                          bool accumulate = false);
int nct_lut_fit_enqueue_masked(nct_ctx* ctx, const char* what, const uint8_t* d_src, const uint8_t* d_res, const uint8_t* d_mask, size_t npix, const nct_lut_params* prm, float* d_lut,
                               const nct_lut_stages* d_stages);
// k_region.hip — source region masks (SPEC §6.11). The single-channel form of nctk_resize_u8c3; the mix of coefficients x ([2][h*w][3]) toward the identity by the level
// mask (x_out may be x); the compose of a finish's Lab result o_lab with the source (BGR and Lab) by the mask at that size, Lab -> BGR in `form` included
int nctk_resize_u8c1(nct_ctx* ctx, hipStream_t s, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);
// the argument checks of nct_resize_u8c1[_dev] (`what` names the entry point in the message)
static inline int nct_resize_u8c1_check(nct_ctx* ctx, const char* what, const void* src, int sh, int sw, const void* dst, int dh, int dw) {
    NCT_REQUIRE(src && dst, "%s: null pointer", what);
    NCT_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0 && sh <= 16384 && sw <= 16384 && dh <= 16384 && dw <= 16384 && (long long)sh * sw <= (1LL << 26) && (long long)dh * dw <= (1LL << 26),
                "%s: size %dx%d -> %dx%d out of range", what, sw, sh, dw, dh);
    return NCT_OK;
}
int nctk_region_mix(nct_ctx* ctx, hipStream_t s, const double* x, const uint8_t* mask, int h, int w, double* x_out);
// the argument checks of nct_region_compose[_dev] (`what` names the entry point in the message)
static inline int nct_region_compose_check(nct_ctx* ctx, const char* what, const void* s_bgr, const void* lab_out, const void* mask, size_t npix, const nct_region_params* region, const nct_params* prm,
                             const void* out_bgr) {
    NCT_REQUIRE(s_bgr && lab_out && mask && prm && out_bgr, "%s: null pointer", what);
    NCT_REQUIRE(npix >= 1 && npix <= (size_t)NCT_FINISH_MAX_PIXELS, "%s: the number of pixels must be in [1, 2^26] (got %zu)", what, npix);
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "%s: region protect must be 0 or 1 (got %d)", what, region ? region->protect : 0);
    return NCT_OK;
}
int nctk_region_compose(nct_ctx* ctx, hipStream_t s, const uint8_t* s_bgr, const uint8_t* s_lab, const uint8_t* o_lab, const uint8_t* mask, size_t npix, int protect, int form,
                        uint8_t* out_bgr);
// SPEC §6.12 rules 3-5. nctk_region_merge: P_l = the pulled mask of the pixel's label (pulled: K device pointers, null = a reference without a mask = 255; label is read
// with K > 1 only) into p_out and M_l = min(P_l, ms) into m_out (ms null = 255; either output nullable). nctk_region_upsize_min: dst = min(resize_u8c1(src -> dh x dw), mn)
// for a target not smaller than the source grid (mn nullable; equal sizes: the copy / the minimum)
int nctk_region_merge(nct_ctx* ctx, hipStream_t s, const uint8_t* const* pulled, int K, const uint8_t* label, const uint8_t* ms, int n, uint8_t* p_out, uint8_t* m_out);
int nctk_region_upsize_min(nct_ctx* ctx, hipStream_t s, const uint8_t* src, int sh, int sw, const uint8_t* mn, uint8_t* dst, int dh, int dw);
// k_wls_mg.hip
int nctk_wls_solve_mg(nct_ctx* ctx, hipStream_t s, double* X, const double* rough, const double* wx, const double* wy, int H, int W,
                      double rtol, int* iters_out);
// pm_mode: how candidate distances are evaluated (k_patchmatch.hip)
enum { NCT_PM_PLAIN = 0,      // fp32 candidate tiles, no rejection (any features)
       NCT_PM_ROWREJECT = 1,  // unit-norm features: exact row-wise early rejection (same NNF and distances as PLAIN) — the pipeline's default
       NCT_PM_FP16 = 2 };     // opt-in reduced-precision mode: fp16 candidate tiles (fp32 accumulate); results differ from fp32
int nctk_patchmatch_bidir(nct_ctx* ctx, hipStream_t s, const float* a_hwc, const float* b_hwc, const void* a_h16, const void* b_h16, int C, int ah, int aw, int bh, int bw,
                          int iters, int rs_max, uint32_t seed_ab, uint32_t seed_ba, uint32_t* ann, float* annd, uint32_t* bnn, float* bnnd,
                          int pm_mode, unsigned long long* counters /*nullable, 4 slots*/);
// k_vote.hip
int nctk_bds_vote_features(nct_ctx* ctx, hipStream_t s, const uint32_t* ann, const uint32_t* bnn, const float* pin_hwc, float* pout_hwc, float* pw /*nullable*/,
                           int C, int ah, int aw, int bh, int bw, float w_coh, float w_comp);
int nctk_bds_vote_image(nct_ctx* ctx, hipStream_t s, const uint8_t* b_bgr, const uint32_t* ann, const uint32_t* bnn,
                        int ah, int aw, int bh, int bw, double w_coh, double w_comp, uint8_t* out_bgr);
int nctk_bds_vote_both(nct_ctx* ctx, hipStream_t s, const uint8_t* b_bgr, const float* pin_hwc, const uint32_t* ann, const uint32_t* bnn, int C,
                       int ah, int aw, int bh, int bw, double w_coh, double w_comp, uint8_t* out_bgr, float* pout_hwc,
                       const uint8_t* q_mask = nullptr /* SPEC §6.12: the reference's level mask (bh x bw), pulled behind the votes through their inversion of bnn … */,
                       uint8_t* pulled = nullptr /* … into this (ah x aw) */);
// reference region masks (SPEC §6.12 rule 2): the pull of the one-byte image q_mask (bh x bw) to the source's grid (out: ah x aw) — B1 on one channel, rounded to
// nearest — through the sorted inverse map and one prefix scan; a level's pull rides behind nctk_bds_vote_both's votes
int nctk_region_pull(nct_ctx* ctx, hipStream_t s, const uint8_t* q_mask, int bh, int bw, const uint32_t* ann, const uint32_t* bnn, int ah, int aw,
                     double w_coh, double w_comp, uint8_t* out);
// the argument checks of nct_region_pull[_dev] (`what` names the entry point in the message)
static inline int nct_region_pull_check(nct_ctx* ctx, const char* what, const void* q_mask, int bh, int bw, const void* ann, const void* bnn, int ah, int aw, const void* out) {
    NCT_REQUIRE(q_mask, "%s: q_mask is null", what);
    NCT_REQUIRE(ann, "%s: ann is null", what);
    NCT_REQUIRE(bnn, "%s: bnn is null", what);
    NCT_REQUIRE(out, "%s: out is null", what);
    NCT_REQUIRE(bh >= 1 && bh <= 4096, "%s: bh = %d is not in [1, 4096]", what, bh);
    NCT_REQUIRE(bw >= 1 && bw <= 4096, "%s: bw = %d is not in [1, 4096]", what, bw);
    NCT_REQUIRE(ah >= 1 && ah <= 4096, "%s: ah = %d is not in [1, 4096]", what, ah);
    NCT_REQUIRE(aw >= 1 && aw <= 4096, "%s: aw = %d is not in [1, 4096]", what, aw);
    return NCT_OK;
}
