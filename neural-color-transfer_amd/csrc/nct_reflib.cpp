// nct_reflib.cpp — reference libraries (SPEC §6.21): the entry points of the int8 descriptor (rule D2), of the match (rule D3) and of nct_reflib, the host object that
// holds a library's rows, with the rank of a source against it (rules D1 to D4). Kernels: k_reflib.hip; the host object and rule D4: nct_reflib_host.h. A context keeps
// the rows of the library it last ranked against on the device (reflib_dev, three arena blocks); every other transient goes back in stream order.
#include "nct_pipeline.h"
#include "nct_reflib_host.h"
#include <atomic>

struct reflib_dev { unsigned long long id = 0, revision = 0; DevBuf<int8_t> rows; DevBuf<int> offsets; DevBuf<float> center; };

void nct_reflib_ctx_free(nct_ctx* ctx) { delete (reflib_dev*)ctx->reflib; ctx->reflib = nullptr; }

// a refusal a host-side rule worded (empty: none) as this context's NCT_ERR_INVALID
static int refuse(nct_ctx* ctx, const std::string& why) { return why.empty() ? NCT_OK : ctx->fail(NCT_ERR_INVALID, "%s", why.c_str()); }
static int refuse_ctxless(const std::string& why) { nct_set_ctxless_error(why.c_str()); return NCT_ERR_INVALID; }

static int quantize8_check(nct_ctx* ctx, const char* who, const void* src, const char* src_name, const void* dst, const char* dst_name, int C, int H, int W) {
    NCT_REQUIRE(src, "%s: null %s", who, src_name);
    NCT_REQUIRE(dst, "%s: null %s", who, dst_name);
    NCT_REQUIRE(C >= 16 && C <= 4096 && (C & 15) == 0, "%s: C must be a multiple of 16 in [16, 4096] (got %d)", who, C);
    NCT_REQUIRE(H >= 1 && W >= 1 && H <= 4096 && W <= 4096, "%s: grid %dx%d out of range", who, W, H);
    return NCT_OK;
}

static int match_check(nct_ctx* ctx, const char* who, const void* a, int na, int C, const void* rows, const int32_t* offsets, int N, const void* fwd, const void* bwd) {
    NCT_REQUIRE(a, "%s: null a", who);
    NCT_REQUIRE(fwd, "%s: null fwd", who);
    NCT_REQUIRE(bwd, "%s: null bwd", who);
    NCT_REQUIRE(na >= 1 && na <= NCT_REFLIB_MAX_ROWS, "%s: na must be in [1, %d] (got %d)", who, NCT_REFLIB_MAX_ROWS, na);
    return refuse(ctx, reflib_table_check(who, C, rows, offsets, N));
}

// the image of nct_reflib_add / nct_reflib_rank and the grid of rule D1
static int image_check(nct_ctx* ctx, const char* who, const nct_reflib* lib, const void* bgr, const char* name, int h, int w) {
    NCT_REQUIRE(lib, "%s: null lib", who);
    NCT_REQUIRE(bgr, "%s: null %s", who, name);
    NCT_REQUIRE(h >= 17 && h <= 4000, "%s: h must be in [17, 4000] (got %d)", who, h);
    NCT_REQUIRE(w >= 17 && w <= 4000, "%s: w must be in [17, 4000] (got %d)", who, w);
    const long long cells = (long long)(((h - 1) >> (lib->tap - 1)) + 1) * (((w - 1) >> (lib->tap - 1)) + 1);
    NCT_REQUIRE(cells <= NCT_REFLIB_MAX_ROWS, "%s: h, w: the grid of tap %d holds %lld cells (at most %d)", who, lib->tap, cells, NCT_REFLIB_MAX_ROWS);
    if (nct_vgg19_weights_info(ctx, nullptr, nullptr, nullptr) != NCT_OK)
        return ctx->fail(NCT_ERR_STATE, "%s: VGG19 weights not loaded (nct_vgg19_load_caffemodel / _load_raw)", who);
    return NCT_OK;
}

// rules D1 and D2 on a device image: the forward stops at the tap, whose own epilogue writes it channel-last; q: [cells][C], the caller's
static int descriptor_of(nct_ctx* ctx, hipStream_t s, const uint8_t* d_bgr, int h, int w, int tap, const float* d_center, int8_t* q) {
    const int C = kTapC[tap - 1], cells = (((h - 1) >> (tap - 1)) + 1) * (((w - 1) >> (tap - 1)) + 1);
    DevBuf<float> feat;
    if (!feat.alloc(ctx, (size_t)cells * C)) return NCT_ERR_HIP;
    float* taps[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    taps[tap - 1] = feat;
    NCT_TRY(nctk_vgg19_forward(ctx, s, d_bgr, h, w, 3 * w, tap, nullptr, nullptr, taps));
    return nctk_feat_quantize8(ctx, s, feat, d_center, q, C, cells);
}

// the context's device copy of the library: nothing moves while the library and its revision are those of the last rank
static int reflib_resident(nct_ctx* ctx, const nct_reflib* L, reflib_dev** out) {
    reflib_dev* D = (reflib_dev*)ctx->reflib;
    if (D && D->id == L->id && D->revision == L->revision) { *out = D; return NCT_OK; }
    nct_reflib_ctx_free(ctx);                                    // the old blocks go back in stream order
    D = new reflib_dev();
    ctx->reflib = D;
    if (!D->rows.alloc(ctx, L->rows.size()) || !D->offsets.alloc(ctx, L->offsets.size()) || (L->centred && !D->center.alloc(ctx, L->center.size()))) {
        nct_reflib_ctx_free(ctx);
        return NCT_ERR_HIP;
    }
    NCT_H2D(D->rows, L->rows.data(), L->rows.size());
    NCT_H2D(D->offsets, L->offsets.data(), sizeof(int32_t) * L->offsets.size());
    if (L->centred) NCT_H2D(D->center, L->center.data(), sizeof(float) * L->center.size());
    NCT_SYNC();
    D->id = L->id; D->revision = L->revision;
    *out = D;
    return NCT_OK;
}

// the offsets of a _dev call: up into a block of the call's and waited for, so that the caller's array is free on return
static int offsets_up(nct_ctx* ctx, const int32_t* offsets, int N, DevBuf<int>& d) {
    if (!d.alloc(ctx, (size_t)N + 1)) return NCT_ERR_HIP;
    NCT_H2D(d, offsets, sizeof(int32_t) * ((size_t)N + 1));
    NCT_SYNC();
    return NCT_OK;
}

static int match_dev_check(nct_ctx* ctx, const char* who, const int8_t* d_a, int na, int C, const int8_t* d_rows, const int32_t* offsets, int N, int64_t* d_fwd, int64_t* d_bwd) {
    NCT_TRY(match_check(ctx, who, d_a, na, C, d_rows, offsets, N, d_fwd, d_bwd));
    NCT_REQUIRE(((uintptr_t)d_a & 15) == 0, "%s: a must be 16-byte aligned", who);
    NCT_REQUIRE(((uintptr_t)d_rows & 15) == 0, "%s: rows must be 16-byte aligned", who);
    NCT_REQUIRE(((uintptr_t)d_fwd & 7) == 0 && ((uintptr_t)d_bwd & 7) == 0, "%s: fwd and bwd must be 8-byte aligned", who);
    return NCT_OK;
}

static std::atomic<unsigned long long> g_next_reflib_id{1};

extern "C" {

void nct_reflib_params_default(nct_reflib_params* p) { if (p) { p->wf = 1; p->wb = 1; } }

// rule D2 alone on a host blob in Caffe's layout: up, to channel-last, one k_feat_quantize8 launch, the rows down
int nct_feat_quantize8(nct_ctx* ctx, const float* src_chw, const float* center, int8_t* dst, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_TRY(quantize8_check(ctx, "feat_quantize8", src_chw, "src_chw", dst, "dst", C, H, W));
    const int HW = H * W; const size_t n = (size_t)C * HW;
    HostCall hc(ctx);
    const float* t = hc.in(src_chw, n);
    const float* mu = hc.in(center, (size_t)C);
    float* x = hc.scratch<float>(n);
    int8_t* y = hc.out(dst, n);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_chw_to_hwc(ctx, ctx->stream, t, x, C, HW));
    NCT_TRY(nctk_feat_quantize8(ctx, ctx->stream, x, mu, y, C, HW));
    return hc.finish();
}

int nct_feat_quantize8_dev(nct_ctx* ctx, const float* d_src_hwc, const float* d_center, int8_t* d_dst, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_TRY(quantize8_check(ctx, "feat_quantize8_dev", d_src_hwc, "d_src_hwc", d_dst, "d_dst", C, H, W));
    NCT_REQUIRE(((uintptr_t)d_src_hwc & 15) == 0 && ((uintptr_t)d_center & 15) == 0, "feat_quantize8_dev: d_src_hwc and d_center must be 16-byte aligned");
    NCT_REQUIRE(((uintptr_t)d_dst & 3) == 0, "feat_quantize8_dev: d_dst must be 4-byte aligned");
    return nctk_feat_quantize8(ctx, ctx->stream, d_src_hwc, d_center, d_dst, C, H * W);
}

// rule D3 alone on host rows: the source, the entries and their offsets up, the three launches, the two sums down
int nct_descriptor_match(nct_ctx* ctx, const int8_t* a, int na, int C, const int8_t* rows, const int32_t* offsets, int N, int64_t* fwd, int64_t* bwd) {
    NCT_CTX_ENTER();
    NCT_TRY(match_check(ctx, "descriptor_match", a, na, C, rows, offsets, N, fwd, bwd));
    const int total = offsets[N];
    HostCall hc(ctx);
    const int8_t *da = hc.in(a, (size_t)na * C), *dr = hc.in(rows, (size_t)total * C);
    const int32_t* dof = hc.in(offsets, (size_t)N + 1);
    long long *df = (long long*)hc.out(fwd, (size_t)N), *db = (long long*)hc.out(bwd, (size_t)N);
    NCT_TRY(hc.ready());
    NCT_TRY(nctk_descriptor_match(ctx, ctx->stream, da, na, C, dr, dof, N, total, df, db));
    return hc.finish();
}

int nct_descriptor_match_dev(nct_ctx* ctx, const int8_t* d_a, int na, int C, const int8_t* d_rows, const int32_t* offsets, int N, int64_t* d_fwd, int64_t* d_bwd) {
    NCT_CTX_ENTER();
    NCT_TRY(match_dev_check(ctx, "descriptor_match_dev", d_a, na, C, d_rows, offsets, N, d_fwd, d_bwd));
    DevBuf<int> dof;
    NCT_TRY(offsets_up(ctx, offsets, N, dof));
    return nctk_descriptor_match(ctx, ctx->stream, d_a, na, C, d_rows, dof, N, offsets[N], (long long*)d_fwd, (long long*)d_bwd);
}

// measurement hook: the mean device time of one match (fill, k_desc_match, k_desc_sums), between two events on the library's stream
int nct_descriptor_match_bench(nct_ctx* ctx, const int8_t* d_a, int na, int C, const int8_t* d_rows, const int32_t* offsets, int N, int64_t* d_fwd, int64_t* d_bwd, int reps,
                               float* kernel_ms) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(kernel_ms, "descriptor_match_bench: null kernel_ms");
    NCT_REQUIRE(reps >= 1 && reps <= 1000, "descriptor_match_bench: reps must be in [1, 1000] (got %d)", reps);
    NCT_TRY(match_dev_check(ctx, "descriptor_match_bench", d_a, na, C, d_rows, offsets, N, d_fwd, d_bwd));
    DevBuf<int> dof;
    NCT_TRY(offsets_up(ctx, offsets, N, dof));
    NCT_TRY(nctk_descriptor_match(ctx, ctx->stream, d_a, na, C, d_rows, dof, N, offsets[N], (long long*)d_fwd, (long long*)d_bwd));   // warm-up
    NCT_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < reps; ++r) NCT_TRY(nctk_descriptor_match(ctx, ctx->stream, d_a, na, C, d_rows, dof, N, offsets[N], (long long*)d_fwd, (long long*)d_bwd));
    NCT_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    NCT_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    NCT_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *kernel_ms = ms / reps;
    return NCT_OK;
}

int nct_reflib_create(int tap, int C, const float* center, nct_reflib** lib) {
    if (!lib) return refuse_ctxless("reflib_create: null lib");
    const std::string why = reflib_tap_check("reflib_create", tap, C);
    if (!why.empty()) return refuse_ctxless(why);
    nct_reflib* L = new nct_reflib();
    L->tap = tap; L->C = C; L->centred = center != nullptr;
    if (center) L->center.assign(center, center + C);
    L->id = g_next_reflib_id.fetch_add(1);
    *lib = L;
    return NCT_OK;
}

int nct_reflib_from_rows(int tap, int C, const float* center, const int8_t* rows, const int32_t* offsets, int N, nct_reflib** lib) {
    if (!lib) return refuse_ctxless("reflib_from_rows: null lib");
    std::string why = reflib_tap_check("reflib_from_rows", tap, C);
    if (why.empty()) why = reflib_table_check("reflib_from_rows", C, rows, offsets, N);
    if (!why.empty()) return refuse_ctxless(why);
    nct_reflib* L = nullptr;
    const int rc = nct_reflib_create(tap, C, center, &L);
    if (rc) return rc;
    L->rows.assign(rows, rows + (size_t)offsets[N] * C);
    L->offsets.assign(offsets, offsets + N + 1);
    L->revision = (unsigned long long)N;
    *lib = L;
    return NCT_OK;
}

int nct_reflib_info(const nct_reflib* lib, int* tap, int* C, int* N, int64_t* total_rows, int* centred) {
    if (!lib) return refuse_ctxless("reflib_info: null lib");
    if (tap) *tap = lib->tap;
    if (C) *C = lib->C;
    if (N) *N = lib->N();
    if (total_rows) *total_rows = lib->total();
    if (centred) *centred = lib->centred ? 1 : 0;
    return NCT_OK;
}

int nct_reflib_rows(const nct_reflib* lib, const int8_t** rows, const int32_t** offsets, const float** center) {
    if (!lib) return refuse_ctxless("reflib_rows: null lib");
    if (rows) *rows = lib->rows.empty() ? nullptr : lib->rows.data();
    if (offsets) *offsets = lib->offsets.data();
    if (center) *center = lib->centred ? lib->center.data() : nullptr;
    return NCT_OK;
}

void nct_reflib_free(nct_reflib* lib) { delete lib; }

// rules D1 and D2 on a host image: one forward to the tap, the rows down and appended
int nct_reflib_add(nct_ctx* ctx, nct_reflib* lib, const uint8_t* bgr, int h, int w) {
    NCT_CTX_ENTER();
    NCT_TRY(image_check(ctx, "reflib_add", lib, bgr, "bgr", h, w));
    const int tap = lib->tap, C = lib->C, cells = (((h - 1) >> (tap - 1)) + 1) * (((w - 1) >> (tap - 1)) + 1);
    NCT_REQUIRE(lib->N() < NCT_REFLIB_MAX_ENTRIES, "reflib_add: lib holds %d entries already", NCT_REFLIB_MAX_ENTRIES);
    NCT_REQUIRE((lib->total() + cells) * C <= NCT_REFLIB_MAX_BYTES, "reflib_add: lib's rows would exceed 2^31 bytes");
    std::vector<int8_t> rows((size_t)cells * C);
    HostCall hc(ctx);
    const uint8_t* ds = hc.in(bgr, (size_t)h * w * 3);
    const float* mu = lib->centred ? hc.in(lib->center.data(), (size_t)C) : nullptr;
    int8_t* q = hc.out(rows.data(), rows.size());
    NCT_TRY(hc.ready());
    NCT_TRY(descriptor_of(ctx, ctx->stream, ds, h, w, tap, mu, q));
    NCT_TRY(hc.finish());
    return refuse(ctx, reflib_append(*lib, "reflib_add", rows.data(), cells));
}

int nct_reflib_rank(nct_ctx* ctx, const nct_reflib* lib, const uint8_t* src_bgr, int h, int w, const nct_reflib_params* params, int32_t* order, int64_t* key, int64_t* fwd,
                    int64_t* bwd) {
    NCT_CTX_ENTER();
    NCT_TRY(image_check(ctx, "reflib_rank", lib, src_bgr, "src_bgr", h, w));
    NCT_REQUIRE(order, "reflib_rank: null order");
    NCT_REQUIRE(lib->N() >= 1, "reflib_rank: lib holds no entry");
    nct_reflib_params p;
    if (params) p = *params; else nct_reflib_params_default(&p);
    NCT_REQUIRE(p.wf >= 0 && p.wf <= 16, "reflib_rank: wf must be in [0, 16] (got %d)", p.wf);
    NCT_REQUIRE(p.wb >= 0 && p.wb <= 16, "reflib_rank: wb must be in [0, 16] (got %d)", p.wb);
    NCT_REQUIRE(p.wf + p.wb > 0, "reflib_rank: wf and wb must not both be 0");
    const int tap = lib->tap, C = lib->C, N = lib->N(), na = (((h - 1) >> (tap - 1)) + 1) * (((w - 1) >> (tap - 1)) + 1);
    reflib_dev* D = nullptr;
    NCT_TRY(reflib_resident(ctx, lib, &D));
    std::vector<long long> f((size_t)N), b((size_t)N), k((size_t)N);
    HostCall hc(ctx);
    const uint8_t* ds = hc.in(src_bgr, (size_t)h * w * 3);
    int8_t* q = hc.scratch<int8_t>((size_t)na * C);
    long long *df = hc.out(f.data(), (size_t)N), *db = hc.out(b.data(), (size_t)N);
    NCT_TRY(hc.ready());
    NCT_TRY(descriptor_of(ctx, ctx->stream, ds, h, w, tap, lib->centred ? (const float*)D->center : nullptr, q));
    NCT_TRY(nctk_descriptor_match(ctx, ctx->stream, q, na, C, D->rows, D->offsets, N, (int)lib->total(), df, db));
    NCT_TRY(hc.finish());
    for (int i = 0; i < N; ++i) k[i] = reflib_key(f[i], b[i], na, lib->offsets[i + 1] - lib->offsets[i], p.wf, p.wb);
    reflib_order(k.data(), N, order);
    for (int i = 0; i < N; ++i) { if (key) key[i] = k[i]; if (fwd) fwd[i] = f[i]; if (bwd) bwd[i] = b[i]; }
    return NCT_OK;
}

int nct_reflib_release(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    nct_reflib_ctx_free(ctx);
    return NCT_OK;
}

}  // extern "C"
