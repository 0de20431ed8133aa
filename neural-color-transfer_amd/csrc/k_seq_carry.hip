// k_seq_carry.hip — correspondence carry of a frame sequence (SPEC §6.23): the kernels that move the kept nearest-neighbour fields of the previous frame along the
// level's backward motion field and merge them into the start field of the level's PatchMatch.
//   k_nnf_carry       rule 3: A'(p) = A(p + m(p)), the 32-bit word copied through the component-wise clamped vector — k_label_carry's rule on words. Its own kernel:
//                     k_label_carry lives beside the held selection and a template over the element would re-instantiate what that file compiles to.
//   k_fwd_min         rule 4: F(s) = min { word(p) : p + m(p) = s }, one atomicMin on a 32-bit word of global memory per source pixel. An integer minimum: the order
//                     in which the adds arrive does not matter. F holds 0xFFFFFFFF (no word has more than 24 bits) from a fill on the stream in front.
//   k_fwd_holes       rule 4: where nothing landed, F(s) = word(clamp(s - m(s))). A thread reads and writes its own element only.
//   k_nnf_remap       rule 4: B'(q) = F(B(q)); the coordinates of B(q) are clamped to F's grid, so a word that does not address it reads inside it.
//   k_nnf_select      rule 6: start(p) = C(p) iff d_C(p) < d_Z(p) as fp32, strictly; a NaN on either side fails the comparison and keeps Z(p). Both directions of a
//                     level in one launch. The distances are step 0 of k_patchmatch.hip, evaluated through nctk_patchmatch[_bidir] with iters = 0 (the fallback of the
//                     two forms: the patch distance is device code of k_patchmatch.hip's own templates and is not reached without moving it) — once for Z, once for C.
// MI355X design: every kernel is one thread per field word, 256 threads per block, 4 B in and 4 B out per thread beside the field; the fields of a 700 x 700 frame's
// finest level are 1.96 MB each, so each launch is a few microseconds of HBM traffic and its cost is the launch. None of this is the hot path: the time the carry saves
// is PatchMatch steps that are not launched.
#include "nct_internal.h"
#include "nct_device.h"

__global__ void __launch_bounds__(256) k_nnf_carry(const uint32_t* __restrict__ prev, int h, int w, const short2* __restrict__ field, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const short2 v = field[i];                                   // (my, mx)
    out[i] = prev[clampi(y + v.x, 0, h - 1) * w + clampi(x + v.y, 0, w - 1)];
}

__global__ void __launch_bounds__(256) k_fwd_min(const short2* __restrict__ field, int h, int w, uint32_t* __restrict__ fwd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const short2 v = field[i];
    atomicMin(&fwd[clampi(y + v.x, 0, h - 1) * w + clampi(x + v.y, 0, w - 1)], xy_pack(x, y));
}

__global__ void __launch_bounds__(256) k_fwd_holes(const short2* __restrict__ field, int h, int w, uint32_t* __restrict__ fwd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    if (fwd[i] != 0xFFFFFFFFu) return;
    const int y = i / w, x = i - y * w;
    const short2 v = field[i];
    fwd[i] = xy_pack(clampi(x - v.y, 0, w - 1), clampi(y - v.x, 0, h - 1));
}

__global__ void __launch_bounds__(256) k_nnf_remap(const uint32_t* __restrict__ bnn, int nb, const uint32_t* __restrict__ fwd, int h, int w, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb) return;
    const uint32_t v = bnn[i];
    out[i] = fwd[min(nnf_y(v), h - 1) * w + min(nnf_x(v), w - 1)];
}

// one direction of the merge; start may be z (every thread reads and writes its own element)
struct MergeJob { const uint32_t* z; const uint32_t* c; const float* dz; const float* dc; uint32_t* start; int n; };

__global__ void __launch_bounds__(256) k_nnf_select(MergeJob j0, MergeJob j1) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool second = i >= j0.n;
    const MergeJob& j = second ? j1 : j0;
    if (second) i -= j0.n;
    if (i >= j.n) return;
    const uint32_t z = j.z[i], c = j.c[i];
    j.start[i] = j.dc[i] < j.dz[i] ? c : z;
}

static bool apart(const void* a, size_t na, const void* b, size_t nb) { return (const char*)a + na <= (const char*)b || (const char*)b + nb <= (const char*)a; }

int nct_nnf_carry_check(nct_ctx* ctx, const char* who, const void* nnf_prev, int h, int w, const void* field, const void* nnf_out) {
    NCT_REQUIRE(nnf_prev && field && nnf_out, "%s: null pointer", who);
    NCT_REQUIRE(h >= 1 && w >= 1 && h < 4096 && w < 4096, "%s: grid %dx%d out of range; NNF coordinates are 12-bit", who, w, h);
    return NCT_OK;
}

int nctk_nnf_carry(nct_ctx* ctx, hipStream_t s, const uint32_t* nnf_prev, int h, int w, const int16_t* field, uint32_t* nnf_out) {
    NCT_TRY(nct_nnf_carry_check(ctx, "nnf_carry", nnf_prev, h, w, field, nnf_out));
    const size_t bytes = sizeof(uint32_t) * (size_t)h * w;
    NCT_REQUIRE(apart(nnf_out, bytes, nnf_prev, bytes), "nnf_carry: nnf_out must not alias nnf_prev");
    hipLaunchKernelGGL(k_nnf_carry, dim3(cdiv(h * w, 256)), dim3(256), 0, s, nnf_prev, h, w, (const short2*)field, nnf_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nct_nnf_forward_map_check(nct_ctx* ctx, const char* who, const void* field, int h, int w, const void* fwd_out) {
    NCT_REQUIRE(field && fwd_out, "%s: null pointer", who);
    NCT_REQUIRE(h >= 1 && w >= 1 && h < 4096 && w < 4096, "%s: grid %dx%d out of range; NNF coordinates are 12-bit", who, w, h);
    return NCT_OK;
}

int nctk_nnf_forward_map(nct_ctx* ctx, hipStream_t s, const int16_t* field, int h, int w, uint32_t* fwd_out) {
    NCT_TRY(nct_nnf_forward_map_check(ctx, "nnf_forward_map", field, h, w, fwd_out));
    const size_t bytes = sizeof(uint32_t) * (size_t)h * w;
    NCT_REQUIRE(apart(fwd_out, bytes, field, bytes), "nnf_forward_map: fwd_out must not alias field");
    // fully written before it is read: the fill, the minimum pass, the hole pass
    NCT_HIP(hipMemsetAsync(fwd_out, 0xFF, bytes, s));
    hipLaunchKernelGGL(k_fwd_min, dim3(cdiv(h * w, 256)), dim3(256), 0, s, (const short2*)field, h, w, fwd_out);
    NCT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fwd_holes, dim3(cdiv(h * w, 256)), dim3(256), 0, s, (const short2*)field, h, w, fwd_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nct_nnf_remap_check(nct_ctx* ctx, const char* who, const void* bnn_prev, int bh, int bw, const void* fwd, int h, int w, const void* bnn_out) {
    NCT_REQUIRE(bnn_prev && fwd && bnn_out, "%s: null pointer", who);
    NCT_REQUIRE(nct_nnf_dims_ok(bh, bw, h, w), "%s: dims out of range (%dx%d -> %dx%d); NNF coordinates are 12-bit", who, bh, bw, h, w);
    return NCT_OK;
}

int nctk_nnf_remap(nct_ctx* ctx, hipStream_t s, const uint32_t* bnn_prev, int bh, int bw, const uint32_t* fwd, int h, int w, uint32_t* bnn_out) {
    NCT_TRY(nct_nnf_remap_check(ctx, "nnf_remap", bnn_prev, bh, bw, fwd, h, w, bnn_out));
    const size_t nb = sizeof(uint32_t) * (size_t)bh * bw, nf = sizeof(uint32_t) * (size_t)h * w;
    NCT_REQUIRE(apart(bnn_out, nb, bnn_prev, nb) && apart(bnn_out, nb, fwd, nf), "nnf_remap: bnn_out must not alias bnn_prev or fwd");
    hipLaunchKernelGGL(k_nnf_remap, dim3(cdiv(bh * bw, 256)), dim3(256), 0, s, bnn_prev, bh * bw, fwd, h, w, bnn_out);
    NCT_LAUNCH_CHECK();
    return 0;
}

int nct_nnf_merge_check(nct_ctx* ctx, const char* who, const void* a, const void* b, int C, int ah, int aw, int bh, int bw, int patch, const void* z, const void* c,
                        const void* start_out) {
    NCT_REQUIRE(a && b && z && c && start_out, "%s: null pointer", who);
    NCT_REQUIRE(patch == 3, "%s: patch must be 3 (Config.h:70), got %d", who, patch);
    NCT_REQUIRE(C > 0 && (C & 3) == 0, "%s: C=%d must be a positive multiple of 4", who, C);
    NCT_REQUIRE(nct_nnf_dims_ok(ah, aw, bh, bw), "%s: dims out of range (%dx%d vs %dx%d); NNF coordinates are 12-bit", who, ah, aw, bh, bw);
    NCT_REQUIRE((long long)C * ah * aw <= NCT_MAX_ELEMS && (long long)C * bh * bw <= NCT_MAX_ELEMS, "%s: a map of %d channels exceeds 2^31 - 256 elements", who, C);
    return NCT_OK;
}

int nctk_nnf_merge(nct_ctx* ctx, hipStream_t s, const float* a_hwc, const float* b_hwc, const void* a_h16, const void* b_h16, int C, int ah, int aw, int bh, int bw, int pm_mode,
                   uint32_t* ann, const uint32_t* ca, float* dza, float* dca, uint32_t* bnn, const uint32_t* cb, float* dzb, float* dcb) {
    NCT_TRY(nct_nnf_merge_check(ctx, "nnf_merge", a_hwc, b_hwc, C, ah, aw, bh, bw, 3, ann, ca, ann));
    NCT_REQUIRE(!bnn || cb, "nnf_merge: null pointer");
    const int na = ah * aw, nb = bnn ? bh * bw : 0;
    // the distance outputs the caller did not ask for are scratch of the call; the blocks go back in stream order
    DevBuf<float> s_dza, s_dca, s_dzb, s_dcb;
    if (!dza) { if (!s_dza.alloc(ctx, na)) return NCT_ERR_HIP; dza = s_dza; }
    if (!dca) { if (!s_dca.alloc(ctx, na)) return NCT_ERR_HIP; dca = s_dca; }
    if (bnn && !dzb) { if (!s_dzb.alloc(ctx, nb)) return NCT_ERR_HIP; dzb = s_dzb; }
    if (bnn && !dcb) { if (!s_dcb.alloc(ctx, nb)) return NCT_ERR_HIP; dcb = s_dcb; }
    // step 0 evaluates the field it is given and leaves it as it is: the candidate fields are read only
    if (bnn) {
        NCT_TRY(nctk_patchmatch_bidir(ctx, s, a_hwc, b_hwc, a_h16, b_h16, C, ah, aw, bh, bw, 0, 0, 0u, 0u, ann, dza, bnn, dzb, pm_mode, nullptr));
        NCT_TRY(nctk_patchmatch_bidir(ctx, s, a_hwc, b_hwc, a_h16, b_h16, C, ah, aw, bh, bw, 0, 0, 0u, 0u, (uint32_t*)ca, dca, (uint32_t*)cb, dcb, pm_mode, nullptr));
    } else {
        NCT_TRY(nctk_patchmatch(ctx, s, a_hwc, b_hwc, C, ah, aw, bh, bw, 0, 0, 0u, ann, dza, nullptr));
        NCT_TRY(nctk_patchmatch(ctx, s, a_hwc, b_hwc, C, ah, aw, bh, bw, 0, 0, 0u, (uint32_t*)ca, dca, nullptr));
    }
    const MergeJob j0{ann, ca, dza, dca, ann, na}, j1{bnn, cb, dzb, dcb, bnn, nb};
    hipLaunchKernelGGL(k_nnf_select, dim3(cdiv(na + nb, 256)), dim3(256), 0, s, j0, j1);
    NCT_LAUNCH_CHECK();
    return 0;
}
