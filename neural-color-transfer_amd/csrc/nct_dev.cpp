// nct_dev.cpp — device-pointer variants of the seams of transfer_color_single_bds (main.cu:204-316): the same launchers the fused per-pair path uses
// (nctk_*), on buffers that STAY in HBM between calls — what an integrator replacing single seams of the reference needs (its own code keeps Ndata_C1,
// ann_device, … on the device across these calls, main.cu:238-326). Host-pointer variants (nct_api.cpp) pay H2D + D2H + a synchronise per call.
// All calls are enqueued on the context's stream in call order and return without waiting; nct_dev_download / nct_synchronize wait.
// Layout: features channel-last (HWC) fp32 — nct_chw_to_hwc_dev converts a Caffe blob once; NNFs u32 (y << 12) | x; images u8 BGR HWC.
#include "nct_internal.h"


extern "C" {

int nct_dev_alloc(nct_ctx* ctx, size_t bytes, void** out) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(out && bytes > 0, "dev_alloc: bad arguments");
    *out = ctx->alloc(bytes);                       // context arena: cached blocks, reused in stream order
    return *out ? NCT_OK : NCT_ERR_HIP;
}
int nct_dev_free(nct_ctx* ctx, void* p) {
    NCT_CTX_ENTER();
    if (!p) return NCT_OK;
    bool mine = false;
    for (const auto& b : ctx->blocks) if (b.p == p && b.used) { mine = true; break; }
    NCT_REQUIRE(mine, "dev_free: %p is not a live nct_dev_alloc block of this context", p);      // a foreign or already freed pointer is an error, not a silent no-op
    ctx->release(p);
    return NCT_OK;
}
int nct_dev_upload(nct_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(dst_dev && src_host, "dev_upload: null pointer");
    NCT_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    NCT_HIP(hipStreamSynchronize(ctx->stream));     // the host buffer may be reused on return
    return NCT_OK;
}
int nct_dev_download(nct_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(dst_host && src_dev, "dev_download: null pointer");
    NCT_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NCT_HIP(hipStreamSynchronize(ctx->stream));
    return NCT_OK;
}

// The argument checks of this family (`who` names the entry point in the message): every seam runs its own in front of the launcher, which reserves and enqueues.
// A map [C][H][W] or [H][W][C]: c_step 4 = the float4 rows of the correspondence kernels, 1 = any C; the sizes fit the launchers' ints
static int map_check(nct_ctx* ctx, const char* who, int C, int H, int W, int c_step) {
    NCT_REQUIRE(C > 0 && C % c_step == 0, "%s: C=%d must be a positive multiple of %d", who, C, c_step);
    NCT_REQUIRE(H > 0 && W > 0, "%s: empty map %dx%d", who, W, H);
    NCT_REQUIRE((long long)H * W <= NCT_MAX_ELEMS && (long long)C * H * W <= NCT_MAX_ELEMS, "%s: a map of %d x %dx%d elements exceeds 2^31 - 256", who, C, W, H);
    return NCT_OK;
}
// a field between two maps
static int field_check(nct_ctx* ctx, const char* who, int ah, int aw, int bh, int bw, int patch) {
    NCT_REQUIRE(patch == 3, "%s: patch must be 3 (Config.h:70), got %d", who, patch);
    NCT_REQUIRE(nct_nnf_dims_ok(ah, aw, bh, bw), "%s: dims out of range (%dx%d vs %dx%d); NNF coordinates are 12-bit", who, ah, aw, bh, bw);
    return NCT_OK;
}
static int pm_check(nct_ctx* ctx, const char* who, int C, int ah, int aw, int bh, int bw, int patch, int iters, int rs_max) {
    NCT_REQUIRE(C > 0 && (C & 3) == 0, "%s: C=%d must be a positive multiple of 4", who, C);
    NCT_TRY(field_check(ctx, who, ah, aw, bh, bw, patch));
    NCT_REQUIRE(iters >= 0 && rs_max >= 0, "%s: iters/rs_max must be >= 0 (got %d, %d)", who, iters, rs_max);
    return NCT_OK;
}
static int image_check(nct_ctx* ctx, const char* who, const void* d_bgr, int h, int w, int stride, int deepest_tap) {
    NCT_REQUIRE(d_bgr, "%s: null pointer", who);
    NCT_REQUIRE(h >= 2 && w >= 2 && h < 4096 && w < 4096, "%s: image size %dx%d out of range", who, w, h);
    NCT_REQUIRE(stride >= 3 * w, "%s: stride %d is less than a row of %d pixels", who, stride, w);
    NCT_REQUIRE(deepest_tap >= 1 && deepest_tap <= 5, "%s: deepest_tap must be 1..5 (got %d)", who, deepest_tap);
    return NCT_OK;
}

int nct_chw_to_hwc_dev(nct_ctx* ctx, const float* src_chw, float* dst_hwc, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(src_chw && dst_hwc, "chw_to_hwc_dev: null pointer");
    NCT_TRY(map_check(ctx, "chw_to_hwc_dev", C, H, W, 1));
    return nctk_chw_to_hwc(ctx, ctx->stream, src_chw, dst_hwc, C, H * W);
}
int nct_hwc_to_chw_dev(nct_ctx* ctx, const float* src_hwc, float* dst_chw, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(src_hwc && dst_chw, "hwc_to_chw_dev: null pointer");
    NCT_TRY(map_check(ctx, "hwc_to_chw_dev", C, H, W, 1));
    return nctk_hwc_to_chw(ctx, ctx->stream, src_hwc, dst_chw, C, H * W);
}

// V2: Classifier::Predict on a device image; taps in Caffe's CHW layout (d_taps_chw[t] nullable)
int nct_vgg19_features_dev(nct_ctx* ctx, const uint8_t* d_bgr, int h, int w, int stride, int deepest_tap, float* const* d_taps_chw, int* dims) {
    NCT_CTX_ENTER();
    NCT_TRY(image_check(ctx, "vgg19_features_dev", d_bgr, h, w, stride, deepest_tap));
    return nctk_vgg19_forward(ctx, ctx->stream, d_bgr, h, w, stride, deepest_tap, d_taps_chw, dims);
}

int nct_vgg19_features_hwc_dev(nct_ctx* ctx, const uint8_t* d_bgr, int h, int w, int stride, int deepest_tap, float* const* d_taps_chw, float* const* d_taps_hwc, int* dims) {
    NCT_CTX_ENTER();
    NCT_TRY(image_check(ctx, "vgg19_features_hwc_dev", d_bgr, h, w, stride, deepest_tap));
    return nctk_vgg19_forward(ctx, ctx->stream, d_bgr, h, w, stride, deepest_tap, d_taps_chw, dims, d_taps_hwc);
}

// One 3x3 / pad 1 / stride 1 conv layer of the VGG stage through the launcher the forward uses (nctk_conv3x3: same dispatch over the four tile forms), every epilogue
// reachable: planar (d_out_chw), channel-last (d_out_hwc), both, or pool = 1 (d_out_chw receives only the 2x2/2 ceil-mode pooled map). d_weights in Caffe layout
// [Cout][Cin][3][3]; packed here into an arena block that goes back in stream order. The kernel consumes channels in pairs: for odd Cin the CALLER's d_in holds Cin + 1
// planes, the last one zero (the packed weights of that channel are zero, but 0 * inf is not) — the forward's preprocess writes conv1_1's fourth plane the same way.
static int conv_pack(nct_ctx* ctx, const float* d_weights, int Cin, int Cout, DevBuf<float>& wp) {
    const int cin_pad = (Cin + 1) & ~1;
    if (!wp.alloc(ctx, (size_t)cin_pad * 9 * Cout)) return NCT_ERR_HIP;
    return nctk_pack_weights(ctx, ctx->stream, d_weights, wp, Cout, Cin, cin_pad);
}
int nct_conv3x3_dev(nct_ctx* ctx, const float* d_in, const float* d_weights, const float* d_bias, int Cin, int Cout, int H, int W, int relu, int pool,
                    float* d_out_chw, float* d_out_hwc) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(d_in && d_weights && d_bias, "conv3x3_dev: null pointer");
    NCT_REQUIRE(Cin >= 1 && Cout >= 64 && H >= 1 && W >= 1 && H < 4096 && W < 4096, "conv3x3_dev: Cin=%d Cout=%d map %dx%d out of range", Cin, Cout, W, H);
    NCT_REQUIRE(d_out_chw || d_out_hwc, "conv3x3: no output");                        // nctk_conv3x3's own refusals, repeated in front of the packing launch
    NCT_REQUIRE(!(pool && d_out_hwc), "conv3x3: the channel-last output exists for un-pooled layers only");
    NCT_REQUIRE((Cout & 63) == 0, "conv3x3: Cout=%d must be a multiple of 64", Cout);
    DevBuf<float> wp;
    NCT_TRY(conv_pack(ctx, d_weights, Cin, Cout, wp));
    return nctk_conv3x3(ctx, ctx->stream, d_in, wp, d_bias, d_out_chw, (Cin + 1) & ~1, Cout, H, W, relu, pool ? 1 : 0, d_out_hwc);
}
// The same layer for two images of different geometry (conv5_1 of the source and the reference in the pipeline): one launch where both grids are small and the context's
// conv_pair switch (NCT_CONV_PAIR) allows it, two launches otherwise — nctk_conv3x3_pair decides, as for the pipeline. Per image one of the two outputs may be null.
int nct_conv3x3_pair_dev(nct_ctx* ctx, const float* d_in1, int H1, int W1, const float* d_in2, int H2, int W2, const float* d_weights, const float* d_bias, int Cin, int Cout,
                         int relu, float* d_out1, float* d_out2, float* d_hwc1, float* d_hwc2) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(d_in1 && d_in2 && d_weights && d_bias, "conv3x3_pair_dev: null pointer");
    NCT_REQUIRE(Cin >= 1 && Cout >= 64 && H1 >= 1 && W1 >= 1 && H2 >= 1 && W2 >= 1 && H1 < 4096 && W1 < 4096 && H2 < 4096 && W2 < 4096,
                "conv3x3_pair_dev: Cin=%d Cout=%d maps %dx%d, %dx%d out of range", Cin, Cout, W1, H1, W2, H2);
    NCT_REQUIRE((d_out1 || d_hwc1) && (d_out2 || d_hwc2), "conv3x3: no output");
    NCT_REQUIRE((Cout & 63) == 0, "conv3x3: Cout=%d must be a multiple of 64", Cout);
    DevBuf<float> wp;
    NCT_TRY(conv_pack(ctx, d_weights, Cin, Cout, wp));
    return nctk_conv3x3_pair(ctx, ctx->stream, d_in1, H1, W1, d_in2, H2, W2, wp, d_bias, d_out1, d_out2, (Cin + 1) & ~1, Cout, relu, d_hwc1, d_hwc2);
}

// N1: norm (main.cu:265,274,313)
int nct_feat_normalize_dev(nct_ctx* ctx, const float* src_hwc, float* dst_hwc, float* resp, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(src_hwc && dst_hwc, "feat_normalize_dev: null pointer");
    NCT_TRY(map_check(ctx, "feat_normalize_dev", C, H, W, 4));
    return nctk_normalize(ctx, ctx->stream, src_hwc, dst_hwc, resp, C, H * W);
}

// N2: init_Ann_kernel / upSample_kernel (main.cu:232-250)
int nct_nnf_init_dev(nct_ctx* ctx, uint32_t* nnf, int ah, int aw, int bh, int bw) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(nnf, "nnf_init_dev: null pointer");
    NCT_REQUIRE(ah >= 2 && aw >= 2 && nct_nnf_dims_ok(ah, aw, bh, bw), "nnf_init_dev: dims out of range (%dx%d -> %dx%d); the query map needs two rows and columns, NNF coordinates are 12-bit",
                ah, aw, bh, bw);
    return nctk_nnf_init(ctx, ctx->stream, nnf, ah, aw, bh, bw);
}
int nct_nnf_upsample_dev(nct_ctx* ctx, const uint32_t* nnf_half, uint32_t* nnf, int ah, int aw, int bh, int bw, int ah_half, int aw_half) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(nnf_half && nnf, "nnf_upsample_dev: null pointer");
    NCT_REQUIRE(nnf_half != nnf, "nnf_upsample_dev: nnf_half and nnf are the same buffer");
    NCT_REQUIRE(nct_nnf_dims_ok(ah, aw, bh, bw) && ah_half >= 1 && aw_half >= 1 && ah_half < 4096 && aw_half < 4096,
                "nnf_upsample_dev: dims out of range (%dx%d from %dx%d -> %dx%d); NNF coordinates are 12-bit", ah, aw, ah_half, aw_half, bh, bw);
    return nctk_nnf_upsample(ctx, ctx->stream, nnf_half, nnf, ah, aw, bh, bw, ah_half, aw_half);
}

// P1: patchmatch_single (main.cu:283-284). One field, or both fields of a level in the same launches (what the pipeline runs).
int nct_patchmatch_dev(nct_ctx* ctx, const float* a_hwc, const float* b_hwc, int C, int ah, int aw, int bh, int bw, int patch, int iters, int rs_max,
                       uint32_t seed, uint32_t* nnf, float* dist) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(a_hwc && b_hwc && nnf && dist, "patchmatch_dev: null pointer");
    NCT_TRY(pm_check(ctx, "patchmatch_dev", C, ah, aw, bh, bw, patch, iters, rs_max));
    return nctk_patchmatch(ctx, ctx->stream, a_hwc, b_hwc, C, ah, aw, bh, bw, iters, rs_max, seed, nnf, dist, nullptr);
}
int nct_patchmatch_bidir_dev(nct_ctx* ctx, const float* a_hwc, const float* b_hwc, int C, int ah, int aw, int bh, int bw, int patch, int iters, int rs_max,
                             uint32_t seed_ab, uint32_t seed_ba, uint32_t* ann, float* annd, uint32_t* bnn, float* bnnd, int unit_norm) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(a_hwc && b_hwc && ann && annd && bnn && bnnd, "patchmatch_bidir_dev: null pointer");
    NCT_TRY(pm_check(ctx, "patchmatch_bidir_dev", C, ah, aw, bh, bw, patch, iters, rs_max));
    return nctk_patchmatch_bidir(ctx, ctx->stream, a_hwc, b_hwc, nullptr, nullptr, C, ah, aw, bh, bw, iters, rs_max, seed_ab, seed_ba, ann, annd, bnn, bnnd,
                                 unit_norm ? NCT_PM_ROWREJECT : NCT_PM_PLAIN, nullptr);
}

// B2 / B1: avg_vote_bds_a/_b/avg_vote_bds, feature_distance, reconstruct_bds (main.cu:291-316)
int nct_bds_vote_features_dev(nct_ctx* ctx, const uint32_t* ann, const uint32_t* bnn, const float* pin_hwc, float* pout_hwc, float* pw, int C, int ah, int aw, int bh, int bw,
                              int patch, float w_coherence, float w_complete) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(ann && bnn && pin_hwc && pout_hwc, "bds_vote_features_dev: null pointer");
    NCT_REQUIRE(C > 0 && (C & 3) == 0 && C <= 512, "bds_vote_features_dev: C=%d must be a multiple of 4 and <= 512", C);
    NCT_TRY(field_check(ctx, "bds_vote_features_dev", ah, aw, bh, bw, patch));
    return nctk_bds_vote_features(ctx, ctx->stream, ann, bnn, pin_hwc, pout_hwc, pw, C, ah, aw, bh, bw, w_coherence, w_complete);
}
int nct_bds_vote_image_dev(nct_ctx* ctx, const uint8_t* b_bgr, const uint32_t* ann, const uint32_t* bnn, int ah, int aw, int bh, int bw, int patch,
                           double w_coherence, double w_complete, uint8_t* out_bgr) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(b_bgr && ann && bnn && out_bgr, "bds_vote_image_dev: null pointer");
    NCT_TRY(field_check(ctx, "bds_vote_image_dev", ah, aw, bh, bw, patch));
    return nctk_bds_vote_image(ctx, ctx->stream, b_bgr, ann, bnn, ah, aw, bh, bw, w_coherence, w_complete, out_bgr);
}
int nct_feature_distance_dev(nct_ctx* ctx, const float* a_hwc, const float* b_hwc, float* err, int C, int H, int W) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(a_hwc && b_hwc && err, "feature_distance_dev: null pointer");
    NCT_TRY(map_check(ctx, "feature_distance_dev", C, H, W, 4));
    return nctk_feature_distance(ctx, ctx->stream, a_hwc, b_hwc, err, C, H * W);
}

int nct_select_reference_dev(nct_ctx* ctx, const float* const* d_err, const uint8_t* const* d_guide_bgr, int K, int h, int w, uint8_t* d_label, uint8_t* d_guide_out,
                             float* d_err_out) {                                                                                                       /* SPEC §6.2 */
    NCT_CTX_ENTER();
    return nctk_select_reference(ctx, ctx->stream, d_err, d_guide_bgr, K, h, w, d_label, d_guide_out, d_err_out);
}

int nct_select_reference_hold_dev(nct_ctx* ctx, const float* const* d_err, const uint8_t* const* d_guide_bgr, int K, int h, int w, const uint8_t* d_prev_label,
                                  const uint8_t* d_lab, const uint8_t* d_lab_prev, const int16_t* d_field, double hold, double sigma, uint8_t* d_label, uint8_t* d_guide_out,
                                  float* d_err_out, uint8_t* d_free_label, double* d_margin) {                                                        /* SPEC §6.18 */
    NCT_CTX_ENTER();
    return nctk_select_hold(ctx, ctx->stream, d_err, d_guide_bgr, K, h, w, d_prev_label, d_lab, d_lab_prev, d_field, hold, sigma, d_label, d_guide_out, d_err_out, d_free_label,
                            d_margin);
}

int nct_seq_pull_hold_dev(nct_ctx* ctx, const uint8_t* const* d_pulled, int K, const uint8_t* d_label, const uint8_t* d_prev, const uint8_t* d_lab, const uint8_t* d_lab_prev,
                          const int16_t* d_field, const uint8_t* d_src_mask, int h, int w, double tau, double sigma, uint8_t* d_p_out, uint8_t* d_m_out, uint8_t* d_p_free) {   /* SPEC §6.19 */
    NCT_CTX_ENTER();
    return nctk_seq_pull_hold(ctx, ctx->stream, d_pulled, K, d_label, d_prev, d_lab, d_lab_prev, d_field, d_src_mask, h, w, tau, sigma, d_p_out, d_m_out, d_p_free);
}

int nct_seq_blend_dev(nct_ctx* ctx, const double* d_x, const double* d_x_prev, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, double tau, double sigma,
                      double* d_x_out, double* d_tau_map) {                                                                                          /* SPEC §6.3 */
    NCT_CTX_ENTER();
    return nctk_seq_blend(ctx, ctx->stream, d_x, d_x_prev, d_lab, d_lab_prev, h, w, tau, sigma, d_x_out, d_tau_map);
}

int nct_seq_blend_mc_dev(nct_ctx* ctx, const double* d_x, const double* d_x_prev, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, double tau, double sigma,
                         double* d_x_out, double* d_tau_map, const int16_t* d_field) {                                                                /* SPEC §6.4 rule 4 */
    NCT_CTX_ENTER();
    return nctk_seq_blend(ctx, ctx->stream, d_x, d_x_prev, d_lab, d_lab_prev, h, w, tau, sigma, d_x_out, d_tau_map, d_field);
}

int nct_seq_warp_dev(nct_ctx* ctx, const double* d_x_prev, int h, int w, const int16_t* d_field, double* d_x_out) {                                /* SPEC §6.5 rule 3 */
    NCT_CTX_ENTER();
    return nctk_seq_warp(ctx, ctx->stream, d_x_prev, h, w, d_field, d_x_out);
}

int nct_seq_matte_warp_dev(nct_ctx* ctx, const uint8_t* d_mask_prev, int H, int W, const int16_t* d_field, int h, int w, uint8_t* d_mask_out) {       /* SPEC §6.14 rule 1 */
    NCT_CTX_ENTER();
    return nctk_seq_matte_warp(ctx, ctx->stream, d_mask_prev, H, W, d_field, h, w, d_mask_out);
}

int nct_region_snap_dev(nct_ctx* ctx, const uint8_t* d_mask, const uint8_t* d_lab, int H, int W, const nct_region_snap_params* params, uint8_t* d_mask_out) {       /* SPEC §6.15 rule 1 */
    NCT_CTX_ENTER();
    return nctk_region_snap(ctx, ctx->stream, d_mask, d_lab, H, W, params, d_mask_out);
}

int nct_seq_change_dev(nct_ctx* ctx, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, const int16_t* d_field, int threshold, nct_seq_change_rec* d_out) {   /* SPEC §6.7 rule 1 */
    NCT_CTX_ENTER();
    return nctk_seq_change(ctx, ctx->stream, d_lab, d_lab_prev, h, w, d_field, threshold, d_out);
}

int nct_seq_motion_field_dev(nct_ctx* ctx, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, const int16_t* d_parent, int ph, int pw, int R, int penalty,
                             int16_t* d_m_out) {                                                                                                      /* SPEC §6.4 rules 1-3 */
    NCT_CTX_ENTER();
    NCT_TRY(nct_seq_motion_field_check(ctx, "seq_motion_field_dev", d_lab, d_lab_prev, h, w, d_parent, ph, pw, d_m_out));
    DevBuf<uint32_t> pk(ctx, (size_t)h * w);                     // L_(t-1) one word per pixel; the block goes back in stream order
    if (!pk.ok()) return NCT_ERR_HIP;
    NCT_TRY(nctk_seq_pack(ctx, ctx->stream, d_lab_prev, h * w, pk));
    return nctk_seq_motion(ctx, ctx->stream, d_lab, pk, h, w, d_parent, ph, pw, R, penalty, d_m_out);
}

// ---- SPEC §6.23 rules 3, 4 and 6 on device pointers
int nct_nnf_carry_dev(nct_ctx* ctx, const uint32_t* d_nnf_prev, int h, int w, const int16_t* d_field, uint32_t* d_nnf_out) {
    NCT_CTX_ENTER();
    return nctk_nnf_carry(ctx, ctx->stream, d_nnf_prev, h, w, d_field, d_nnf_out);
}

int nct_nnf_forward_map_dev(nct_ctx* ctx, const int16_t* d_field, int h, int w, uint32_t* d_fwd_out) {
    NCT_CTX_ENTER();
    return nctk_nnf_forward_map(ctx, ctx->stream, d_field, h, w, d_fwd_out);
}

int nct_nnf_remap_dev(nct_ctx* ctx, const uint32_t* d_bnn_prev, int bh, int bw, const uint32_t* d_fwd, int h, int w, uint32_t* d_bnn_out) {
    NCT_CTX_ENTER();
    return nctk_nnf_remap(ctx, ctx->stream, d_bnn_prev, bh, bw, d_fwd, h, w, d_bnn_out);
}

int nct_nnf_merge_dev(nct_ctx* ctx, const float* d_a_hwc, const float* d_b_hwc, int C, int ah, int aw, int bh, int bw, int patch, const uint32_t* d_z, const uint32_t* d_c,
                      uint32_t* d_start_out, float* d_dz_out, float* d_dc_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_nnf_merge_check(ctx, "nnf_merge_dev", d_a_hwc, d_b_hwc, C, ah, aw, bh, bw, patch, d_z, d_c, d_start_out));
    const size_t bytes = sizeof(uint32_t) * (size_t)ah * aw;
    const auto apart = [bytes](const void* p, const void* q) { return (const char*)p + bytes <= (const char*)q || (const char*)q + bytes <= (const char*)p; };
    NCT_REQUIRE(apart(d_start_out, d_z) && apart(d_start_out, d_c), "nnf_merge_dev: start_out must not alias z or c");
    // Z into the output, which the launcher then merges in place
    NCT_HIP(hipMemcpyAsync(d_start_out, d_z, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return nctk_nnf_merge(ctx, ctx->stream, d_a_hwc, d_b_hwc, nullptr, nullptr, C, ah, aw, bh, bw, NCT_PM_PLAIN, d_start_out, d_c, d_dz_out, d_dc_out, nullptr, nullptr, nullptr, nullptr);
}

// ---- SPEC §6.11 on device pointers
int nct_resize_u8c1_dev(nct_ctx* ctx, const uint8_t* d_src, int sh, int sw, uint8_t* d_dst, int dh, int dw) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_resize_u8c1_check(ctx, "resize_u8c1_dev", d_src, sh, sw, d_dst, dh, dw));
    return nctk_resize_u8c1(ctx, ctx->stream, d_src, sh, sw, d_dst, dh, dw);
}

int nct_region_mix_dev(nct_ctx* ctx, const double* d_x, const uint8_t* d_mask, int h, int w, double* d_x_out) {
    NCT_CTX_ENTER();
    return nctk_region_mix(ctx, ctx->stream, d_x, d_mask, h, w, d_x_out);
}

int nct_region_compose_dev(nct_ctx* ctx, const uint8_t* d_s_bgr, const uint8_t* d_lab_out, const uint8_t* d_mask, size_t npix, const nct_region_params* region,
                           const nct_params* prm, uint8_t* d_out_bgr) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_compose_check(ctx, "region_compose_dev", d_s_bgr, d_lab_out, d_mask, npix, region, prm, d_out_bgr));
    DevBuf<uint8_t> ls(ctx, npix * 3);                           // Lab_S; the block goes back in stream order
    if (!ls.ok()) return NCT_ERR_HIP;
    NCT_TRY(nctk_bgr2lab(ctx, ctx->stream, d_s_bgr, ls, npix));
    return nctk_region_compose(ctx, ctx->stream, d_s_bgr, ls, d_lab_out, d_mask, npix, region ? region->protect : 0, (prm->flags & NCT_FLAG_LAB2BGR_CUBE) ? 1 : 0, d_out_bgr);
}

// ---- SPEC §6.12 rule 2 on device pointers
int nct_region_pull_dev(nct_ctx* ctx, const uint8_t* d_q_mask, int bh, int bw, const uint32_t* d_ann, const uint32_t* d_bnn, int ah, int aw, double w_coherence,
                        double w_complete, uint8_t* d_out) {
    NCT_CTX_ENTER();
    NCT_TRY(nct_region_pull_check(ctx, "region_pull_dev", d_q_mask, bh, bw, d_ann, d_bnn, ah, aw, d_out));
    return nctk_region_pull(ctx, ctx->stream, d_q_mask, bh, bw, d_ann, d_bnn, ah, aw, w_coherence, w_complete, d_out);
}

// ---- the upsampling finish on device pointers, in its four forms (SPEC §6.8, §6.10, §6.13 rule 4); mask NULL is the unmasked call. The form's name is nctk_finish_up's
static int finish_up_dev(nct_ctx* ctx, bool is_guided, const double* d_ab_wls, const uint8_t* d_lab_work, int h, int w, const uint8_t* d_s_bgr_full, int H, int W, const uint8_t* d_mask,
                         const nct_region_params* region, const nct_guided_params* guided, const nct_params* prm, uint8_t* d_out_bgr_full) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(prm && (guided || !is_guided), "%s_dev: null pointer", nct_finish_up_name(is_guided, d_mask != nullptr));
    char who[64];
    snprintf(who, sizeof who, "%s_dev", nct_finish_up_name(is_guided, d_mask != nullptr));
    NCT_TRY(nct_params_check(ctx, who, *prm));
    const nct_finish_up up{d_s_bgr_full, H, W, d_out_bgr_full, nct_cube_form(*prm), is_guided ? guided->sigma : 0.0, d_mask, region ? region->protect : 0};
    NCT_TRY(nctk_finish_up_check(ctx, is_guided, d_ab_wls, d_lab_work, h, w, up));      // a guided call is never read as a plain one, whatever its sigma
    return nctk_finish_up(ctx, ctx->stream, d_ab_wls, d_lab_work, h, w, up);
}

int nct_color_finish_upsample_dev(nct_ctx* ctx, const double* d_ab_wls, int h, int w, const uint8_t* d_s_bgr_full, int H, int W, const nct_params* prm, uint8_t* d_out_bgr_full) {
    return finish_up_dev(ctx, false, d_ab_wls, nullptr, h, w, d_s_bgr_full, H, W, nullptr, nullptr, nullptr, prm, d_out_bgr_full);
}

int nct_color_finish_guided_dev(nct_ctx* ctx, const double* d_ab_wls, const uint8_t* d_lab_work, int h, int w, const uint8_t* d_s_bgr_full, int H, int W,
                                const nct_guided_params* guided, const nct_params* prm, uint8_t* d_out_bgr_full) {
    return finish_up_dev(ctx, true, d_ab_wls, d_lab_work, h, w, d_s_bgr_full, H, W, nullptr, nullptr, guided, prm, d_out_bgr_full);
}

int nct_color_finish_upsample_region_dev(nct_ctx* ctx, const double* d_ab_wls, int h, int w, const uint8_t* d_s_bgr_full, int H, int W, const uint8_t* d_mask,
                                         const nct_region_params* region, const nct_params* prm, uint8_t* d_out_bgr_full) {
    return finish_up_dev(ctx, false, d_ab_wls, nullptr, h, w, d_s_bgr_full, H, W, d_mask, region, nullptr, prm, d_out_bgr_full);
}

int nct_color_finish_guided_region_dev(nct_ctx* ctx, const double* d_ab_wls, const uint8_t* d_lab_work, int h, int w, const uint8_t* d_s_bgr_full, int H, int W,
                                       const uint8_t* d_mask, const nct_region_params* region, const nct_guided_params* guided, const nct_params* prm, uint8_t* d_out_bgr_full) {
    return finish_up_dev(ctx, true, d_ab_wls, d_lab_work, h, w, d_s_bgr_full, H, W, d_mask, region, guided, prm, d_out_bgr_full);
}

}  // extern "C"
