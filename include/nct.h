/* include/nct.h — C ABI of libnct.so: the MI355X-native hot path of Neural-Color-Transfer.
 *
 * The reference (hmmlillian/Neural-Color-Transfer) has no plugin/FFI layer: the path is reached through
 * ordinary C++ calls and kernel launches inside `transfer_color_single_bds`
 * (code/windows/neural_color_transfer/source/main.cu:47-454). Each entry point below replaces one seam of
 * that function; the seam is cited as `main.cu:<line>` (+ the kernel/function it launches).
 *
 * Conventions
 *  - plain C, no C++/torch types. Every function returns 0 on success, <0 on error (nct_status);
 *    `nct_last_error(ctx)` returns a human-readable message for the last failure on that context.
 *  - a context is bound to ONE GPU and is NOT thread-safe; use one context per worker thread / process.
 *    The context owns every device allocation (cached arena, reused across calls and pairs).
 *  - "host" entry points take host pointers and are synchronous. Feature tensors are CHW fp32 exactly like the
 *    reference kernels' arguments (`float* a1`, Caffe blob layout). The `*_dev` variants (section "device-pointer seams"
 *    below) work on device pointers in the library's internal channel-last (HWC) layout and do not synchronise.
 *  - NNF element = uint32 `(y << 12) | x` (GeneralizedPatchMatch.cu:24-34), row-major (ah x aw).
 *  - there is NO CPU fallback: without a usable HIP device nct_create fails with NCT_ERR_NO_DEVICE.
 */
#ifndef NCT_H
#define NCT_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever a struct of this header changes layout or an entry point changes meaning (round 6: 110 — nct_model_layer; nct_pair_timing grew in round 5 without a
 * bump; 111 — nct_multi_levels and the entry points for several references; 112 — frame sequences, nct_seq_*; 113 — nct_seq_levels.motion and motion-compensated
 * sequences, nct_seq_set_motion; 114 — propagated frames, nct_seq_frame_propagate and nct_seq_warp; 115 — the single-layer conv seams nct_conv3x3_dev and
 * nct_conv3x3_pair_dev; 116 — 3D colour look-up tables, nct_lut_*; 117 — adaptive key frames, nct_seq_change, nct_seq_probe and nct_seq_frame_auto; 118 — the upsampling finish and
 * full-resolution sequences, nct_color_finish_upsample, nct_process_pair_fullres_finish and nct_seq_begin_fullres; still 118 with the guided finish, nct_color_finish_guided[_dev], nct_set_finish_guided and nct_guided_params: no struct
 * changed layout and no existing entry point changed meaning, entry points were only added; likewise still 118 with source region masks, nct_region_*, nct_pair_set_region,
 * nct_process_pair_region and nct_lut_fit_masked, and with reference region masks, nct_region_pull[_dev], nct_pair_set_ref_region, nct_multi_run_ref_region_levels and
 * nct_process_*_ref_region, and with region masks in sequences, nct_seq_set_region, nct_seq_frame[_propagate]_region_levels and nct_color_finish_{upsample,guided}_region[_dev], and with region tracking,
 * nct_seq_matte_warp[_dev], nct_seq_set_region_tracking and nct_seq_get_region, and with matte snapping, nct_region_snap[_dev], nct_region_snap_params and
 * nct_seq_set_region_snap, and with region selection from strokes, nct_region_select[_dev], nct_feat_quantize[_dev], nct_region_score[_dev], nct_pair_select_region and
 * nct_seq_select_region, and with region models, nct_region_model_*, nct_region_refind[_dev], nct_pair_apply_region_model and nct_seq_set_region_model, and with sequences
 * over several references, nct_seq_begin_multi[_fullres], nct_seq_frame_multi[_stage]_levels, nct_seq_hold, nct_seq_hold_levels and nct_select_reference_hold[_dev], and with reference
 * region masks in sequences, nct_seq_set_ref_region, nct_seq_pull_hold[_dev], nct_seq_pull_levels and nct_seq_frame[_propagate]_ref_region_levels, and with shot look-up tables and the 16-bit apply,
 * nct_lut_accum_* and nct_lut_apply_u16[_dev], and with local colour grids, nct_grid_* and nct_pair_fit_grid, and
 * with the correspondence carry of sequences, nct_seq_set_carry, nct_seq_get_carry and nct_nnf_{carry,forward_map,remap,merge}[_dev]).
 * A caller checks `nct_version() == NCT_VERSION` before it passes any struct: the CLI
 * and the python binding do. */
#define NCT_VERSION 118

typedef enum {
    NCT_OK = 0,
    NCT_ERR_NO_DEVICE = -1,     /* no HIP device / hipInit failed (fail loudly, no fallback) */
    NCT_ERR_INVALID = -2,       /* bad argument (null pointer, size out of range, unsupported C/patch) */
    NCT_ERR_HIP = -3,           /* a HIP runtime call or kernel launch failed */
    NCT_ERR_IO = -4,            /* file not found / unreadable / malformed */
    NCT_ERR_STATE = -5          /* call order (e.g. features before weights are loaded) */
} nct_status;

typedef struct nct_ctx nct_ctx;

/* ---- context (replaces cudaSetDevice/cudaDeviceReset + the two Classifier objects, main.cu:562-584) ---- */
int nct_create(int device, nct_ctx** out);
void nct_destroy(nct_ctx* ctx);
const char* nct_last_error(const nct_ctx* ctx);     /* ctx may be NULL: returns the last create() failure */
int nct_version(void);
int nct_device_name(nct_ctx* ctx, char* buf, int buflen);
/* no context needed: number of visible HIP devices, and a device's PCI address "dddd:bb:dd.f" — the key of /sys/bus/pci/devices/<addr>/numa_node and
 * local_cpulist, which the CLI pins a GPU's worker threads to ("worker thread pinned to the GPU's NUMA node") */
int nct_device_count(int* count);
int nct_device_pci_bus_id(int device, char* buf, int buflen);
int nct_synchronize(nct_ctx* ctx);
/* counters of a context (what library code must not print): NCT_CTR_ARENA_BYTES = device memory held by the context's arena; NCT_CTR_S1_HUB_BLOCKS_L0 + l (l = 0 coarsest … 4) =
 * the number of in-edge blocks beyond a pixel's first 64 in level l's kNN graph of the LAST pair, as the host knew it when it enqueued that level's nonlocal solve
 * (0 on the synthetic pairs; thousands on natural photographs, where groups of one colour make kNN hubs — k_s1.hip; -1: not known in time, the hub pass was launched anyway). */
enum { NCT_CTR_ARENA_BYTES = 0, NCT_CTR_S1_HUB_BLOCKS_L0 = 1 };
int nct_ctx_counter(nct_ctx* ctx, int which, int64_t* out);

/* ---- N1: feature L2 normalisation — `norm` (GeneralizedPatchMatch.cu:237-283), called main.cu:265,274,313.
 * dst = src / sqrt(sum_c src^2) per pixel (no epsilon, like the reference). resp (nullable, H*W) receives the
 * min-max normalised response map (|x| - min)/(max - min). C must be a multiple of 4. */
int nct_feat_normalize(nct_ctx* ctx, const float* src_chw, float* dst_chw, float* resp, int C, int H, int W);

/* ---- N2: NNF initialisation / upsampling — init_Ann_kernel (:527-544), upSample_kernel (:546-580);
 * launched main.cu:232-233 and :240-250. */
int nct_nnf_init(nct_ctx* ctx, uint32_t* nnf, int ah, int aw, int bh, int bw);
int nct_nnf_upsample(nct_ctx* ctx, const uint32_t* nnf_half, uint32_t* nnf, int ah, int aw, int bh, int bw, int ah_half, int aw_half);

/* ---- P1: PatchMatch — patchmatch_single (:677-831), launched main.cu:283-284 (S->R) and (R->S).
 * a/b: L2-normalised CHW features of the query / candidate image. nnf: in/out. dist: out (ah*aw), the
 * negative mean cosine of the best match. patch must be 3 (Config.h:70), C a multiple of 4.
 * Deterministic: Jacobi step per (iteration, jump), counter-based RNG keyed by `seed`. */
int nct_patchmatch(nct_ctx* ctx, const float* a_chw, const float* b_chw, int C, int ah, int aw, int bh, int bw,
                   int patch, int iters, int rs_max, uint32_t seed, uint32_t* nnf, float* dist);

/* ---- B2: feature-domain BDS vote + matching error — avg_vote_bds_a/_b/avg_vote_bds (:1074-1202),
 * feature_distance (:833-855); launched main.cu:303-316.
 * pin: UN-normalised R features (C,bh,bw). pout: voted features (C,ah,aw). pw (nullable): accumulated weights. */
int nct_bds_vote_features(nct_ctx* ctx, const uint32_t* ann, const uint32_t* bnn, const float* pin_chw, float* pout_chw, float* pw,
                          int C, int ah, int aw, int bh, int bw, int patch, float w_coherence, float w_complete);
int nct_feature_distance(nct_ctx* ctx, const float* a_chw, const float* b_chw, float* err, int C, int H, int W);

/* ---- B1: image-domain BDS vote — reconstruct_bds (GeneralizedPatchMatch.cu:122-235), called main.cu:291.
 * a, b: u8 BGR HWC level images of S and R; out: guidance image G (ah x aw x 3). */
int nct_bds_vote_image(nct_ctx* ctx, const uint8_t* a_bgr, int ah, int aw, const uint8_t* b_bgr, int bh, int bw,
                       const uint32_t* ann, const uint32_t* bnn, int patch, double w_coherence, double w_complete, uint8_t* out_bgr);

/* ---- V1: VGG19 weights — Classifier::Classifier (Classifier.cpp:5-42) -> Net::CopyTrainedLayersFrom
 * (code/src/caffe/net.cpp:760-813). Reads a .caffemodel (protobuf wire format, V1 `layers`=2 as in the Oxford file, or
 * V2 `layer`=100), matches conv layers BY NAME, ignores unknown layers, fails on a shape mismatch. Only conv1_1..conv5_1
 * (13 layers) are required/uploaded. _load_raw takes Caffe-layout arrays [Cout][Cin][3][3] + [Cout] in net order. */
int nct_vgg19_load_caffemodel(nct_ctx* ctx, const char* path);
int nct_vgg19_load_raw(nct_ctx* ctx, const float* const* weights, const float* const* biases, int nlayers);
/* A driver with several contexts (the CLI's -gpus N -inflight K; main.cu:581-582 builds two Nets from the file): parse the 575 MB file ONCE per process into a
 * host-side model (52 MB: the 13 needed layers), upload it ONCE per GPU (nct_vgg19_load_model), and let the other contexts of that GPU use the same read-only
 * device copy (nct_vgg19_share_weights; both contexts must live on the same device; the copy is freed with its last user). nct_model_* need no context;
 * nct_model_last_error() returns the message of the last failed parse on the calling thread. nct_vgg19_weights_info: identity (device address of conv1_1's
 * packed weights), size in bytes and number of contexts sharing this context's copy. */
typedef struct nct_model nct_model;
int nct_model_parse_caffemodel(const char* path, nct_model** out);
void nct_model_free(nct_model* m);
/* read access to a parsed model (host memory, valid until nct_model_free): layer 0..12 = conv1_1 .. conv5_1 in net order; weights [cout][cin][3][3], bias [cout].
 * What Net::CopyTrainedLayersFrom leaves in the layer's blobs (net.cpp:776-792) — lets a caller (and the CPU tests) check an ingest without a device. */
int nct_model_layer(const nct_model* m, int layer, const float** weights, const float** bias, int* cout, int* cin);
const char* nct_model_last_error(void);
int nct_vgg19_load_model(nct_ctx* ctx, const nct_model* m);
int nct_vgg19_share_weights(nct_ctx* ctx, nct_ctx* from);
int nct_vgg19_weights_info(nct_ctx* ctx, uint64_t* id, size_t* bytes, int* sharers);
/* Classifier::Classifier builds its Net from <model_dir>/vgg19/VGG_ILSVRC_19_layers_deploy.prototxt (Classifier.cpp:16; main.cu:575-577). This library's
 * topology is built in, so the file is only checked (protobuf text format, `layer` or V1 `layers` messages): conv1_1..conv5_1 in order with the built-in
 * channel counts, 3x3 / pad 1 / stride 1, each followed by an in-place ReLU, 2x2 / stride-2 MAX pools after conv1_2, 2_2, 3_4, 4_4. Anything else ->
 * NCT_ERR_IO with a message (ctx nullable: then through nct_model_last_error). Layers behind relu5_1 are not looked at. */
int nct_vgg19_check_prototxt(nct_ctx* ctx, const char* path);

/* ---- V2/R1: VGG19 features — Classifier::Predict (Classifier.cpp:59-143), called main.cu:94,102,426.
 * bgr: u8 BGR HWC image (row stride in bytes). Runs preprocess (mean subtraction, Classifier.cpp:211-275) and the net
 * up to tap `deepest_tap` (1 = conv1_1 … 5 = conv5_1; the reference always runs to pool5, SURVEY quirk 9 — the
 * result is identical). taps_chw[t] (nullable entries) receives the post-ReLU blob of tap t+1 in Caffe's CHW layout;
 * dims (nullable, int[15]) receives {C,H,W} per tap. */
int nct_vgg19_features(nct_ctx* ctx, const uint8_t* bgr, int h, int w, int stride, int deepest_tap, float* const* taps_chw, int* dims);

/* single layers (unit parity against Caffe's known-answer tests): 3x3 pad-1 stride-1 conv + bias (+ ReLU) on f32 MFMA
 * (conv_layer.cpp:8-40; Cout % 64 == 0), 2x2/2 MAX pool with ceil-mode size (pooling_layer.cpp:90-93,147-165). */
int nct_conv3x3_relu(nct_ctx* ctx, const float* in_chw, int Cin, int H, int W, const float* weights, const float* bias, int Cout, float* out_chw, int relu);
int nct_maxpool2x2(nct_ctx* ctx, const float* in_chw, int C, int H, int W, float* out_chw);

/* ---- parameters: `Config` (ColorTransfer/Config.h:55-98) + the constants hard-coded in transfer_color_single_bds
 * (main.cu:64-68: iter = 10). nct_params_default fills Config::Config()'s values (bds 2.0, eps 0.60, nl 2.0, l 0.125,
 * w 0.024, clusters 10, k 8, patch 3, alpha 1.2) — the help strings at main.cu:40-43 quote different numbers; the
 * constructor is what runs. `seed` keys the counter-based RNG (PatchMatch random search, k-means centres).
 * The solvers' domain: eps, nonlocal_weight, local_weight, wls_lambda_init and wls_alpha must each be finite and > 0 (T1 divides by eps, S1 and S2 take roots of the
 * weights, and |dL|^wls_alpha is evaluated for an exponent > 0 only), bds_weight finite and >= 0; cluster_num lies in [1, 16], k_num is 8 and patch_size 3. Every entry
 * point that takes the struct returns NCT_ERR_INVALID for anything else, with a message that names the field, before it enqueues anything. */
typedef struct nct_params {
    double bds_weight, eps, nonlocal_weight, local_weight, wls_lambda_init;
    int cluster_num, k_num, patch_size;
    double wls_alpha;
    int pm_iters;
    uint32_t seed;
    int levels;         /* pyramid levels to run, coarse -> fine: 5 = the reference's full L=5..1 loop (main.cu:179); 1 = "L=5 only"
                           (BASELINE config 1): the result is the full-resolution image after the coarsest level's colour transfer */
    uint32_t flags;     /* NCT_FLAG_* (extensions; 0 = reference behaviour) */
} nct_params;
#define NCT_FLAG_FEAT16      1u   /* opt-in reduced precision: PatchMatch reads fp16 candidate feature tiles (fp32 accumulate). Halves the
                                     dominant kernel's bytes; the result is NOT bit-identical to the fp32 path (report PSNR against it) */
#define NCT_FLAG_COUNT_EVALS 2u   /* profiling: count PatchMatch evaluations per level on the device (nct_pair_timing.pm_level_evals …) */
#define NCT_FLAG_LATENCY     4u   /* one pair in flight on this GPU: spend extra launches on its latency — the a- and b-halves of each WLS solve
                                     run concurrently on two streams. Same result bit for bit; with several pairs in flight it only adds launches */
#define NCT_FLAG_LAB2BGR_CUBE 8u  /* CV_Lab2BGR in the older plain-cube form of OpenCV's Lab2RGB_f (no linear branch, no clipping) instead of the default piecewise
                                     form — see nct_lab2bgr_u8_form for which one the reference's own result images show */
#define NCT_FLAG_TIME_KERNELS 16u /* profiling: HIP events around single launches of the finest level's colour-solver kernels (nct_pair_timing.kernel_us); the
                                     extra events perturb the pair a little: use a run of its own */
void nct_params_default(nct_params* p);

/* ---- A1 + third-party (OpenCV 2.4.10) arithmetic used on the path: cvtColor(CV_BGR2Lab / CV_Lab2BGR) on 8U
 * (main.cu:352,371; ColorTransfer.h:58; ColorTransfer.cpp:1469) and cv::resize(INTER_LINEAR) on 8UC3 / 64FC3
 * (main.cu:106-107; ColorTransfer.cpp:462-463; includes cv::resize's silent INTER_AREA switch for an exact 2x shrink). */
int nct_bgr2lab_u8(nct_ctx* ctx, const uint8_t* bgr, size_t npix, uint8_t* lab);
int nct_lab2bgr_u8(nct_ctx* ctx, const uint8_t* lab, size_t npix, uint8_t* bgr);      /* = form NCT_LAB2BGR_PIECEWISE */
/* The two forms of Lab2RGB_f in OpenCV's history (the sources of the pinned 2.4.10 cannot be inspected here — SURVEY App. A):
 * NCT_LAB2BGR_PIECEWISE (default): CIE's linear branch below L* = 8 / f = 6/29 and linear RGB clipped to [0, 1]; NCT_LAB2BGR_CUBE: fY = (L+16)/116,
 * fX = fY + a/500, fZ = fY - b/200, all cubed, linear RGB NOT clipped (the inverse-gamma spline extrapolates, the final cast saturates).
 * The default is decided by the reference's own artefacts: the cube form cannot produce a pixel darker than (9, 9, 9) on the grey axis nor (0, 0, 0) at
 * all (Y >= (16/116)^3 > 0), yet demo/example/res/in0_tar0_2.00.png holds 415 pixels with all channels < 5 incl. (0, 0, 0) and every result image with
 * dark regions has pixels like (0, 2, 0) = the linear branch at L_u8 = 1..2 (tests/golden/demo_res_dark_stats.json). */
#define NCT_LAB2BGR_PIECEWISE 0
#define NCT_LAB2BGR_CUBE 1
int nct_lab2bgr_u8_form(nct_ctx* ctx, const uint8_t* lab, size_t npix, uint8_t* bgr, int form);
int nct_resize_u8c3(nct_ctx* ctx, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);
int nct_resize_f64c3(nct_ctx* ctx, const double* src, int sh, int sw, double* dst, int dh, int dw);

/* ---- C1: k-means labels of the coarsest S features — main.cu:139-168 -> ColorTransfer::clusterFeastures
 * (ColorTransfer.cpp:355-395; cvflann k-means, branching K, `iters` Lloyd steps). feat_chw: UN-normalised conv5_1 of S;
 * labels: h*w ints in [0, *nlabels). K lies in [1, 16]. K == 1 is this library's own rule, not the reference's, whose FLANN refuses a branching below 2
 * (Flann/kmeans_index.h:370-372): one cluster, every label 0, *nlabels = 1. */
int nct_cluster_features(nct_ctx* ctx, const float* feat_chw, int C, int h, int w, int K, int iters, uint64_t seed, int* labels, int* nlabels);

/* ---- K1: kNN graph in Lab — ColorTransfer::findKnns (ColorTransfer.cpp:397-423), called main.cu:359.
 * lab_u8: level image in 8-bit Lab (HWC); labels: coarsest-level cluster labels (lh x lw); samples = 2^level.
 * knn_id / knn_w: [h*w][k] neighbour ids and weights exp(1 - d/3); k must be 8. */
int nct_knn_graph(nct_ctx* ctx, const uint8_t* lab_u8, int h, int w, const int* labels, int lh, int lw, int nlabels, int samples, int k,
                  int* knn_id, double* knn_w);

/* ---- T1,T2,S1,U1,S2,A1: build_accumTable_downsample x2 + transfer_color_downsample + getRes
 * (ColorTransfer.cpp:425-455,1180-1478), called main.cu:368-380. err: matching-error map of the level (h x w);
 * s_bgr_level / g_bgr_level: level images of S and the BDS guidance G; s_bgr_full: S at full resolution (H x W);
 * layer = 0 (coarsest) … 4 (finest). out: recoloured S (H x W x 3, BGR). `stages` (nullable) receives intermediate
 * coefficient maps for stage-wise validation: arrays are [2][pixels][3] doubles (a-part then b-part). */
typedef struct nct_color_stages {
    double* ab_local;      /* [2][h*w][3]  after the local statistics (T1)            */
    double* ab_nonlocal;   /* [2][h*w][3]  after the truncated CG (S1)                */
    double* ab_up;         /* [2][H*W][3]  after bilinear upsampling (U1)             */
    double* roughness;     /* [H*W]                                                   */
    double* ab_wls;        /* [2][H*W][3]  after WLS smoothing (S2)                   */
    int* cg_iters;         /* [3]  CG iterations executed per Lab channel             */
    int* wls_iters;        /* [6]  PCG iterations per right-hand side                 */
} nct_color_stages;
int nct_local_color_transfer(nct_ctx* ctx, const float* err, const uint8_t* s_bgr_level, const uint8_t* g_bgr_level, const uint8_t* s_bgr_full,
                             const int* knn_id, const double* knn_w, int layer, int h, int w, int H, int W, const nct_params* prm,
                             uint8_t* out_bgr_full, nct_color_stages* stages);

/* ---- D3: the per-pair hot loop — transfer_color_single_bds (main.cu:47-454): VGG19 features of S and R, k-means of
 * S's conv5_1, then for L = 5..1: NNF init/upsample, normalise, PatchMatch both ways, BDS votes, matching error, kNN
 * graph, local colour transfer, re-predict. Images are 8-bit BGR, tightly packed HWC. out has the size of src.
 * `timing` (nullable) receives per-stage device milliseconds under the reference's own stage names (main.cu:331,453;
 * ColorTransfer.cpp:1373,1434), taken from events on the stream (no extra host synchronisation).
 * nct_process_pair = nct_pair_upload + nct_pair_run + nct_pair_download; the split form lets a caller keep inputs
 * resident in HBM (bench.py times nct_pair_run only and reports the PCIe-inclusive rate separately). */
typedef struct nct_pair_timing {
    double total_ms;                    /* host wall time of nct_pair_run */
    /* device time between stage-boundary events on the pair's main stream; read once after the pair has finished, so asking for
       timing does not add host synchronisation (the kNN graphs run on a side stream: knn_ms is only what the main stream waited) */
    double vgg_ms, cluster_ms, patchmatch_ms, vote_ms, knn_ms, color_ms, other_ms;
    double nonlocal_ms, wls_ms;         /* parts of color_ms: S1 = "Nonlocal Solve Time" (ColorTransfer.cpp:1373), S2 = "WLS Solve Time" (:1434) */
    int wls_iters[5];                   /* PCG iterations of the WLS solve per level */
    /* PatchMatch per pyramid level (0 = coarsest): kernel time of the level's launches (init + pm_iters*4 steps, both directions per launch) */
    double pm_level_ms[5];
    int pm_level_launches[5];
    double vote_level_ms[5], nonlocal_level_ms[5], wls_level_ms[5];   /* the same split per level, for the reference's per-level log lines */
    unsigned long long pm_level_evals[5], pm_level_accepted[5];   /* NCT_FLAG_COUNT_EVALS only, else 0: distance evaluations, accepted candidates */
    /* NCT_FLAG_TIME_KERNELS only, else 0: average microseconds per launch (HIP events on the pair's stream around kernel_samples[i] single launches) of the
       colour-solver kernels at full resolution — index NCT_KT_*: the operator pass, the one-workgroup scalar step and the vector pass of the finest level's truncated CG (S1), and the WLS
       PCG's finest V-cycle legs, operator + dot products, vector update, and everything below the finest level of one V-cycle */
    double kernel_us[10];
    int kernel_samples[10];
} nct_pair_timing;
enum { NCT_KT_S1_APPLY = 0, NCT_KT_S1_SCALARS = 1, NCT_KT_S1_UPDATE = 2, NCT_KT_WLS_DOWN = 3, NCT_KT_WLS_UP = 4, NCT_KT_WLS_APPLY = 5, NCT_KT_WLS_UPDATE = 6, NCT_KT_WLS_COARSE = 7,
       NCT_KT_WLS_BLOCK_PRE = 8, NCT_KT_WLS_BLOCK_POST = 9 /* the block step of alternating line solves in front of the finest down leg / behind the finest up leg */ };
/* per-level intermediates for level-wise validation (all pointers nullable; level 0 = coarsest … 4 = finest; arrays have the level's
 * size ah*aw / bh*bw except `result`, the full-resolution intermediate result after that level, H*W*3 like level_out of the oracle) */
typedef struct nct_pair_levels {
    uint32_t* ann[5]; uint32_t* bnn[5];
    float* annd[5]; float* bnnd[5];
    uint8_t* guide[5];
    float* err[5];
    uint8_t* result[5];
    const nct_color_stages* color[5];   /* the colour stage's coefficient maps of the level (T1 / S1 / U1 / S2), as nct_local_color_transfer returns them */
    int* labels;                        /* [ah0*aw0] k-means labels of S's deepest features (the kNN graphs' clusters); level 0's size */
} nct_pair_levels;
int nct_process_pair(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, const nct_params* prm,
                     uint8_t* out_bgr, nct_pair_timing* timing);
int nct_pair_upload(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw);
int nct_pair_run(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing);
int nct_pair_run_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels);   /* + host copies of the intermediates */
int nct_pair_download(nct_ctx* ctx, uint8_t* out_bgr);

/* ---- full-resolution output (SPEC §6.1; an extension: the reference returns every image shrunk to MAX_SIZE, main.cu:500-522).
 * nct_working_size (no context; the message of a refusal is nct_last_error(NULL)): the size the pyramid runs at — unchanged if both sides are <= max_side,
 * else the longer side becomes max_side and the other (int)(max_side / (float)long * short). Refused with NCT_ERR_INVALID: max_side outside [17, 4000],
 * a side above 16384, more than 2^26 pixels, a working side below 17.
 * nct_process_pair_fullres: both images are shrunk by that rule on the device, every level runs as nct_process_pair runs it on the shrunk pair, except
 * that the last level's U1 / S2 / A1 target the ORIGINAL source: out has sh x sw pixels. A source that is not shrunk gives nct_process_pair's result.
 * nct_pair_timing: the finish's WLS counts in wls_ms / wls_level_ms[levels-1] and wls_iters[levels-1], the rest of it in color_ms.
 * nct_color_finish: that finish alone, on host buffers: ab = nct_color_stages.ab_nonlocal of a level of h x w in a pyramid of working size
 * work_h x work_w, s_bgr_full the source at H x W (>= h x w). stages (nullable) receives ab_up, roughness, ab_wls and wls_iters. */
int nct_working_size(int h, int w, int max_side, int* work_h, int* work_w);
int nct_process_pair_fullres(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, int max_side,
                             const nct_params* prm, uint8_t* out_bgr /* sh x sw x 3 */, nct_pair_timing* timing);
int nct_color_finish(nct_ctx* ctx, const double* ab, int h, int w, int work_h, int work_w, const uint8_t* s_bgr_full, int H, int W, const nct_params* prm,
                     uint8_t* out_bgr_full, nct_color_stages* stages);

/* ---- the upsampling finish (SPEC §6.8; an extension). The exact finish above costs one WLS solve at the original size. The upsampling finish runs the last level's
 * finish at the working size as nct_process_pair does, then takes that finish's smoothed coefficient maps (nct_color_stages.ab_wls, [2][h*w][3]), upsamples them to
 * the original size with U1's arithmetic (nct_resize_f64c3; equal sizes: a copy) and applies them to the original pixels with A1's: per original pixel
 * Lab = nct_bgr2lab_u8(S0), v = Lab / 255 * a + b clamped to [0, 1], rint(v * 255), then Lab -> BGR in the form NCT_FLAG_LAB2BGR_CUBE selects. One kernel, 3 B read
 * and 3 B written per original pixel, no original-size intermediate; byte for byte the chain nct_bgr2lab_u8 -> nct_resize_f64c3 x2 -> A1 -> nct_lab2bgr_u8.
 * nct_color_finish_upsample: host pointers, synchronous; 1 <= h <= H <= 16384, 1 <= w <= W <= 16384, at most 2^26 pixels each. nct_color_finish_upsample_dev: the same on
 * device pointers, enqueued on the context's stream. A null pointer, a grid out of range or a target smaller than the grid: NCT_ERR_INVALID with a message.
 * nct_process_pair_fullres_finish: nct_process_pair_fullres with the finish chosen. NCT_FINISH_EXACT is nct_process_pair_fullres (which calls this). With
 * NCT_FINISH_UPSAMPLE every level, the last level's working-size S2 included, runs as nct_process_pair runs it on the shrunk pair; the rule above then gives the
 * sh x sw result. A source that is not shrunk gives nct_process_pair's bytes for either finish; any other `finish` is NCT_ERR_INVALID. nct_pair_timing: wls_* then
 * count the working-size solve, the upsampling pass counts in color_ms. nct_pair_fit_lut afterwards reads the original source and the full result. */
enum { NCT_FINISH_EXACT = 0, NCT_FINISH_UPSAMPLE = 1 };
int nct_color_finish_upsample(nct_ctx* ctx, const double* ab_wls, int h, int w, const uint8_t* s_bgr_full, int H, int W, const nct_params* prm, uint8_t* out_bgr_full);
int nct_color_finish_upsample_dev(nct_ctx* ctx, const double* d_ab_wls, int h, int w, const uint8_t* d_s_bgr_full, int H, int W, const nct_params* prm,
                                  uint8_t* d_out_bgr_full);
int nct_process_pair_fullres_finish(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* ref_bgr, int rh, int rw, int max_side, int finish,
                                    const nct_params* prm, uint8_t* out_bgr /* sh x sw x 3 */, nct_pair_timing* timing);

/* ---- the guided finish (SPEC §6.10; an extension): the upsampling finish made edge-aware, a MODIFIER of NCT_FINISH_UPSAMPLE and not a third finish. S2 is edge-aware,
 * so ab_wls jumps at object boundaries and the bilinear stretch above smears every jump over the original-to-working ratio in original pixels. The guided finish is the
 * joint-bilateral upsampling: per original pixel, with L = nct_bgr2lab_u8(S0) and (s, f) the source index and fraction of nct_resize's bilinear rule per axis, the
 * 4 x 4 working-size taps (s_y + j, s_x + k), j, k = -1 .. 2 (j outer), that lie inside the grid get the weight
 *     g = (1 - |f_y - j| / 2) (1 - |f_x - k| / 2) / (1 + d2 / sigma^2),    d2 = the integer squared distance of L and lab_work(tap) over the three bytes,
 * a tap whose spatial weight is exactly 0 is skipped (a NaN coefficient there stays out), a = sum g a(tap) / sum g, b likewise, in tap order in double, then A1 and
 * Lab -> BGR as above. lab_work: the 8-bit Lab image of the WORKING-size source (h*w*3, nct_bgr2lab_u8 of the shrunk source). sigma: finite and > 0, in 8-bit Lab
 * units, its square finite and > 0 as well; default 10. Equal sizes give nct_color_finish_upsample's bytes. One kernel, 3 B read and 3 B written per original
 * pixel, no original-size intermediate. nct_color_finish_guided: host pointers, synchronous; nct_color_finish_guided_dev: device pointers, enqueued on the context's
 * stream. Limits and refusals as nct_color_finish_upsample; a bad sigma is NCT_ERR_INVALID.
 * nct_set_finish_guided: non-null turns the modifier on for this context, NULL turns it off (the default); a bad sigma is NCT_ERR_INVALID and leaves the setting as
 * it was. It may be called at any time, also while a sequence is open, and takes effect with the next finish that is enqueued. While it is on, every upsampling
 * finish behind a working-size finish runs guided, with that finish's own Lab image as the guide and no further device memory: nct_process_pair_fullres_finish(...,
 * NCT_FINISH_UPSAMPLE, ...) and the full, propagated and auto frames of nct_seq_begin_fullres(..., NCT_FINISH_UPSAMPLE, ...). Unaffected: NCT_FINISH_EXACT,
 * nct_color_finish_upsample[_dev] themselves, sources that need no shrinking and everything at the working size (a sequence's state, probes, decisions). */
typedef struct nct_guided_params { double sigma; } nct_guided_params;
void nct_guided_params_default(nct_guided_params* p);
int nct_color_finish_guided(nct_ctx* ctx, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, int H, int W, const nct_guided_params* guided,
                            const nct_params* prm, uint8_t* out_bgr_full);
int nct_color_finish_guided_dev(nct_ctx* ctx, const double* d_ab_wls, const uint8_t* d_lab_work, int h, int w, const uint8_t* d_s_bgr_full, int H, int W,
                                const nct_guided_params* guided, const nct_params* prm, uint8_t* d_out_bgr_full);
int nct_set_finish_guided(nct_ctx* ctx, const nct_guided_params* guided);

/* ---- several references (SPEC §6.2; an extension: the paper describes it, the reference ships the single-reference form only).
 * Every level runs nct_pair_run's correspondence once per reference R_k (its own NNFs, its own random-search radius max(H, W, RH_k, RW_k), the single-pair seeds),
 * which gives K guidance images G_k and matching errors E_k on the source's level grid. The selection then labels every pixel with the reference whose error,
 * summed over the 3 x 3 window in double (NaN = 0.0, taps outside the grid skipped, dy outer / dx inner), is smallest — the lowest index on a tie — and merges
 * G and E by that label; the rest of the level (Lab, kNN graph, T1 … A1, re-predict) runs once, unchanged. K = 1 is nct_process_pair byte for byte and
 * enqueues the same launches; a list that repeats one image gives the K = 1 result and the label 0 everywhere.
 * nct_select_reference: the selection alone. err[k]: h*w fp32, guide_bgr[k]: h*w*3; label (h*w), guide_out (h*w*3), err_out (h*w; the selected fp32 WORD, a NaN
 * stays that NaN) are all nullable. Host pointers, synchronous; the _dev form takes device pointers (the two arrays OF pointers are host memory: they travel
 * in the kernel's argument block) and is enqueued on the context's stream like the other device-pointer seams.
 * nct_multi_upload / _run / _run_levels / nct_process_multi mirror the nct_pair_* calls; every image obeys nct_pair_upload's limits, 1 <= K <= NCT_MAX_REFS,
 * anything else is NCT_ERR_INVALID with a message. nct_pair_download fetches the result of either form. nct_pair_timing: patchmatch_ms, vote_ms,
 * pm_level_ms[l] and pm_level_launches[l] are sums over the references; the selection counts as vote time. */
#define NCT_MAX_REFS 8
/* per-level intermediates of a run with several references (all pointers nullable; sizes as in nct_pair_levels, per reference k < K its own bh*bw) */
typedef struct nct_multi_levels {
    uint32_t* ann[NCT_MAX_REFS][5]; uint32_t* bnn[NCT_MAX_REFS][5];
    float* annd[NCT_MAX_REFS][5]; float* bnnd[NCT_MAX_REFS][5];
    uint8_t* ref_guide[NCT_MAX_REFS][5];   /* G_k */
    float* ref_err[NCT_MAX_REFS][5];       /* E_k */
    uint8_t* label[5];                     /* [ah*aw] the selected reference per pixel */
    uint8_t* guide[5];                     /* merged G */
    float* err[5];                         /* merged E */
    uint8_t* result[5];
    int* labels;                           /* k-means labels, as in nct_pair_levels */
} nct_multi_levels;
int nct_select_reference(nct_ctx* ctx, const float* const* err, const uint8_t* const* guide_bgr, int K, int h, int w, uint8_t* label, uint8_t* guide_out, float* err_out);
int nct_select_reference_dev(nct_ctx* ctx, const float* const* d_err, const uint8_t* const* d_guide_bgr, int K, int h, int w, uint8_t* d_label, uint8_t* d_guide_out,
                             float* d_err_out);
int nct_multi_upload(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw);
int nct_multi_run(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing);
int nct_multi_run_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_multi_levels* levels);
int nct_process_multi(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, const nct_params* prm,
                      uint8_t* out_bgr, nct_pair_timing* timing);

/* ---- frame sequences (SPEC §6.3; an extension: the reference treats every pair on its own, so the frames of a clip graded to one reference flicker).
 * A sequence is one reference, one nct_params (copied at begin), a temporal weight tau in [0, 1), a sensitivity sigma > 0 (8-bit Lab units) and frames of one size
 * sh x sw. Every frame runs nct_pair_run's level loop on (S_t, R) unchanged, with one insertion per level between S1 and U1: S1's coefficients X_t are blended with
 * the coefficients X'_(t-1) that went into the previous frame's finish, X'_t = X_t + tau_p (X'_(t-1) - X_t), tau_p = tau / (1 + qbar / sigma^2), qbar = the mean squared
 * difference of the two frames' 8-bit Lab level images over the pixel's 3 x 3 window (integer sum, dy outer / dx inner, taps outside the grid skipped, divided by
 * 3 * taps); a NaN in X'_(t-1) leaves X_t. X'_t replaces S1's output in U1 / roughness / S2 / A1 and so in the next level's re-predict. Frame 0, the first frame
 * after nct_seq_reset and every frame with tau == 0 enqueue no blend and equal nct_process_pair(S_t, R) byte for byte.
 * nct_seq_begin prepares the reference once (upload, pyramid, one VGG19 forward: its five taps stay on the device) and reserves the per-level state (X': 48 B,
 * L: 3 B per level pixel); all of it lives in the context's arena until nct_seq_end / nct_destroy. While a sequence is open nct_pair_upload, nct_multi_upload,
 * nct_process_pair_fullres and what is built on them return NCT_ERR_STATE. tau outside [0, 1), a sigma that is not finite and positive or an image outside
 * nct_pair_upload's limits is NCT_ERR_INVALID; nct_seq_frame without an open sequence NCT_ERR_STATE. A frame that fails leaves the sequence reset.
 * nct_seq_frame_levels: nct_pair_levels as in nct_pair_run_levels — color[l]->ab_nonlocal is S1's output BEFORE the blend, ab_up / roughness / ab_wls come after
 * it; nct_seq_levels adds X'_t and the tau_p map per level (a frame without a blend reports X_t and 0.0). The blend's time counts in nct_pair_timing.color_ms.
 * nct_seq_blend: the blend alone on host maps (synchronous), x / x_prev / x_out [2][h*w][3], lab / lab_prev h*w*3 (8-bit Lab), tau_map (nullable) h*w;
 * nct_seq_blend_dev: the same on device pointers, enqueued on the context's stream (x_out may be x or x_prev: every thread reads its pixel before it writes it).
 * Motion compensation (SPEC §6.4): nct_seq_begin opens a sequence without it. nct_seq_set_motion, on an open sequence between frames, turns it on from the next frame
 * (radius0 in [0, 8], radius in [0, 3], penalty in [0, 255]; out of range NCT_ERR_INVALID, no open sequence NCT_ERR_STATE) and reserves 8 B per level pixel more;
 * NULL or both radii 0 turns it off and gives that back: every byte and every launch is then the plain sequence's. On a frame that blends, every level first finds
 * per pixel the displacement m(p) = (my, mx) into the previous frame's Lab level image — a 5 x 5 block match, integer SAD over the three Lab bytes, searched
 * radius0 around (0, 0) at the first level run and radius around twice the coarser level's vector elsewhere, key = cost + penalty * taps * (|dy| + |dx|), compared
 * as cost per tap — and the blend reads L_(t-1) (for qbar: 3 x 3 taps inside the grid in both frames) and X'_(t-1) at p + m(p). Identical frames give m = 0.
 * nct_seq_levels.motion: the field per level, int16 [h*w][2]; a level without one (motion off, no blend) reports zeros.
 * nct_seq_motion_field / _dev: the search alone. lab / lab_prev h*w*3, parent (nullable: the centre is (0, 0)) the coarser field int16 [ph*pw][2], R in [0, 8],
 * m_out int16 [h*w][2]. nct_seq_blend_mc / _dev: nct_seq_blend with a nullable field; with one, x_out must not be x_prev (the blend gathers from other pixels), and a
 * vector that leaves the grid is clamped to it.
 * Propagated frames (SPEC §6.5): nct_seq_frame_propagate runs a frame of the open sequence without the pair's level loop. Per level run it takes the frame's 8-bit Lab
 * level image L_t (the pyramid and cvtColor of a full frame), finds the field m of §6.4 on (L_t, L_(t-1)) while motion is on (m = 0 while it is off) and moves the kept
 * coefficients along it, X'_t(p) = X'_(t-1)(p + m(p)): the 64-bit words are copied, a NaN stays that NaN. X'_t, L_t and the packed map replace the previous frame's, so a
 * later nct_seq_frame blends against a propagated frame as against any other. The result is the finish of the last level run alone — nct_color_finish(X'_t[levels-1],
 * h, w, sh, sw, S_t) — on the frame's own pixels. No VGG forward, normalise, NNF, PatchMatch, vote, k-means, kNN graph, T1, T2, S1 or re-predict is enqueued; tau and
 * sigma play no part. A frame identical to the previous one returns the previous frame's bytes. Which frames are full ("key frames") is the caller's choice; a sequence
 * that never propagates is unchanged in bytes, launches and arena size: the one scratch map the warp needs (48 B per pixel of the last level run, only with motion on) is
 * reserved by the first propagated frame. No open sequence, or one without state (the first frame after nct_seq_begin / nct_seq_reset): NCT_ERR_STATE; a null image:
 * NCT_ERR_INVALID; a refused call changes nothing, a frame that fails later leaves the sequence reset.
 * nct_pair_timing of a propagated frame: vgg_ms, patchmatch_ms, vote_ms, knn_ms and pm_level_launches[] are 0; the finish counts in color_ms / wls_ms /
 * wls_level_ms[levels-1] / wls_iters[levels-1]. nct_seq_frame_propagate_levels reports through nct_seq_levels: ab_blend[l] = X'_t[l], motion[l] = the field (zeros with
 * motion off), tau_map[l] = 1.0 everywhere (the previous frame's weight).
 * nct_seq_warp: the warp alone on host maps (synchronous): x_prev / x_out [2][h*w][3], field int16 [h*w][2] of (my, mx); a vector that leaves the grid is first clamped
 * component-wise so that p + m is inside. nct_seq_warp_dev: the same on device pointers, enqueued; x_out must not overlap x_prev (the warp gathers): NCT_ERR_INVALID. */
typedef struct nct_seq_params { double tau, sigma; } nct_seq_params;
void nct_seq_params_default(nct_seq_params* p);     /* tau 0.7, sigma 10.0 */
typedef struct nct_seq_levels { double* ab_blend[5]; double* tau_map[5]; int16_t* motion[5]; } nct_seq_levels;   /* X'_t [2][h*w][3]; tau_p [h*w]; m [h*w][2]; all nullable */
typedef struct nct_seq_motion { int radius0, radius, penalty; } nct_seq_motion;
void nct_seq_motion_default(nct_seq_motion* p);     /* 3, 1, 1 */
int nct_seq_set_motion(nct_ctx* ctx, const nct_seq_motion* motion);
int nct_seq_begin(nct_ctx* ctx, const uint8_t* ref_bgr, int rh, int rw, int sh, int sw, const nct_params* prm, const nct_seq_params* seq);
/* Full-resolution sequences (SPEC §6.9): nct_seq_begin_fullres opens a sequence whose reference and frames arrive at their ORIGINAL size (limits: nct_working_size's).
 * Both are shrunk on the device by nct_working_size's rule with nct_resize_u8c3's arithmetic — the reference once, every frame when it arrives. Until nct_seq_end every
 * frame call above and below (nct_seq_frame, _levels, _propagate, _propagate_levels, nct_seq_probe, nct_seq_frame_auto) takes sh x sw originals and returns sh x sw
 * bytes. Everything the sequence keeps — X', L, packed maps, fields, the counters — lives on the working-size level grids and equals, word for word, the state of
 * nct_seq_begin(shrunk reference, working size) fed the shrunk frames, for either finish: probe records and nct_seq_frame_auto's decisions are that sequence's. Only
 * the finish of the last level run differs: NCT_FINISH_EXACT — nct_color_finish(X'_t[top], h, w, work_h, work_w, S0_t); NCT_FINISH_UPSAMPLE — the working-size finish,
 * then nct_color_finish_upsample of its ab_wls onto S0_t. With NCT_FINISH_EXACT a first frame (and a frame after nct_seq_reset) equals nct_process_pair_fullres byte for
 * byte; with frames that need no shrinking every call returns the nct_seq_begin sequence's bytes. nct_seq_frame_levels: `levels` must be NULL (its result[] arrays have
 * no single size: NCT_ERR_INVALID), seq_levels reports the working-size maps. The original frame and its result stay in the arena for the life of the sequence
 * (nct_pair_fit_lut reads them); the exact finish's transients go back after every frame. A bad finish or max_side or a size outside the limits: NCT_ERR_INVALID. */
int nct_seq_begin_fullres(nct_ctx* ctx, const uint8_t* ref_bgr, int rh, int rw, int sh, int sw, int max_side, int finish, const nct_params* prm, const nct_seq_params* seq);
int nct_seq_frame(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing);
int nct_seq_frame_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_seq_levels* seq_levels);
int nct_seq_frame_propagate(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing);
int nct_seq_frame_propagate_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels);
int nct_seq_reset(nct_ctx* ctx);   /* scene cut: the next frame is a first frame; the reference stays prepared */
int nct_seq_end(nct_ctx* ctx);     /* frees the state; nct_destroy does it too */
int nct_seq_blend(nct_ctx* ctx, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                  double* x_out, double* tau_map);
int nct_seq_blend_dev(nct_ctx* ctx, const double* d_x, const double* d_x_prev, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, double tau, double sigma,
                      double* d_x_out, double* d_tau_map);
int nct_seq_motion_field(nct_ctx* ctx, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, const int16_t* parent, int ph, int pw, int R, int penalty, int16_t* m_out);
int nct_seq_motion_field_dev(nct_ctx* ctx, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, const int16_t* d_parent, int ph, int pw, int R, int penalty,
                             int16_t* d_m_out);
int nct_seq_blend_mc(nct_ctx* ctx, const double* x, const double* x_prev, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, double tau, double sigma,
                     double* x_out, double* tau_map, const int16_t* field);
int nct_seq_blend_mc_dev(nct_ctx* ctx, const double* d_x, const double* d_x_prev, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, double tau, double sigma,
                         double* d_x_out, double* d_tau_map, const int16_t* d_field);
int nct_seq_warp(nct_ctx* ctx, const double* x_prev, int h, int w, const int16_t* field, double* x_out);
int nct_seq_warp_dev(nct_ctx* ctx, const double* d_x_prev, int h, int w, const int16_t* d_field, double* d_x_out);

/* ---- frame sequences over several references, with a held selection (SPEC §6.18; an extension). C ABI and python only: the console driver has no option for it.
 * nct_seq_begin_multi / nct_seq_begin_multi_fullres open a sequence over K references, 1 <= K <= NCT_MAX_REFS, every image within the limits of nct_seq_begin /
 * nct_seq_begin_fullres (rh / rw: K heights and widths). Each reference is prepared as nct_seq_begin prepares its one: upload (shrunk on the device in the
 * full-resolution form), pyramid, one VGG19 forward, five taps kept. nct_seq_begin[_fullres] is the K = 1 case: bytes, launches and arena requests are the same.
 * Every level of a full frame runs SPEC §6.2 rule 1 per reference, then a selection, then §6.2 rule 3's merge; the rest of the level, the blend of §6.3 / §6.4 and the
 * finish (either full-resolution finish too) are those of a sequence over one reference. The sequence keeps one more map per level run: the label map l_t, one byte
 * per level pixel. The selection is §6.2 rule 2 unchanged, with no new launch, on a first frame, on the frame after nct_seq_reset or a cut, on every frame when
 * tau == 0, hold == 0 or K == 1. On every other full frame, per level pixel p, in IEEE double, uncontracted, in this order:
 *   1. score_k(p) as in §6.2 rule 2; n(p) = the window taps inside the grid; f = the lowest k of the smallest score;
 *   2. m(p) = the level's field of §6.4 while motion is on, clamped component-wise so that p + m is inside the grid, else 0; j = l_(t-1)(p + m(p));
 *   3. g(p) = the g of §6.3 rule 3 (§6.4 rule 4 with a field) on L_t[l] and the kept L_(t-1)[l], operation for operation;
 *   4. margin = (hold * g) * (double)n;
 *   5. l_t(p) = f if j >= K or score_f < score_j - margin (strictly), else j;
 *   6. the merge is §6.2 rule 3 with l_t, and l_t replaces the kept map (out of place: the rule gathers).
 * hold is in units of matching error per window tap (E = -cos in [-1, 1]), finite and in [0, 2]; a NULL nct_seq_hold gives nct_seq_hold_default's. Where the frame did
 * not change, a pixel keeps the label it had along the motion until another reference is better by more than hold per tap; where it changed, g -> 0 and the selection is
 * free. With motion on the level's field is found once, in front of the selection, and the blend reads that field. A propagated frame carries the labels,
 * l_t(p) = l_(t-1)(p + m(p)) (left as they are with motion off); a later full frame holds against them like against any other.
 * nct_seq_frame, nct_seq_frame_propagate[_levels], nct_seq_probe, nct_seq_frame_auto, nct_seq_reset, nct_seq_end, nct_seq_set_motion and the region calls of
 * §6.13-§6.17 work unchanged (a source mask acts behind the merge, §6.2 rule 5). nct_seq_frame_levels with a non-null nct_pair_levels is NCT_ERR_INVALID for K > 1:
 * nct_seq_frame_multi_levels reports through nct_multi_levels (label[l] = l_t; in a full-resolution sequence its result[] must be NULL), nct_seq_levels and
 * nct_seq_hold_levels — free_label[l] = f ([h*w] bytes), margin[l] = rule 4's value ([h*w] doubles), on a frame without a hold f = l_t and 0.0; all nullable.
 * nct_seq_frame_multi_stage_levels also takes color[5] (nullable, each nullable), the colour stage's maps per level as nct_pair_levels.color reports them.
 * nct_pair_set_ref_region and nct_multi_upload stay NCT_ERR_STATE while a sequence is open; reference masks in sequences: SPEC §6.19, nct_seq_set_ref_region.
 * nct_select_reference_hold: rules 1-6 alone on host maps (synchronous). err[k] h*w fp32, guide_bgr[k] h*w*3, prev_label h*w, lab / lab_prev h*w*3 (8-bit Lab), field
 * (nullable: m = 0) int16 [h*w][2]; label, guide_out, err_out (as in nct_select_reference), free_label (h*w) and margin (h*w doubles) are nullable. The _dev form takes
 * device pointers (the two arrays OF pointers are host memory) and is enqueued on the context's stream; there label must not overlap prev_label. K outside
 * [1, NCT_MAX_REFS], a grid outside 1 … 4096 per side, a null input, hold outside [0, 2] or not finite, sigma not finite and positive: NCT_ERR_INVALID. */
typedef struct nct_seq_hold { double hold; } nct_seq_hold;
void nct_seq_hold_default(nct_seq_hold* p);         /* hold 0.005 */
typedef struct nct_seq_hold_levels { uint8_t* free_label[5]; double* margin[5]; } nct_seq_hold_levels;
int nct_seq_begin_multi(nct_ctx* ctx, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, int sh, int sw, const nct_params* prm, const nct_seq_params* seq,
                        const nct_seq_hold* hold);
int nct_seq_begin_multi_fullres(nct_ctx* ctx, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, int sh, int sw, int max_side, int finish,
                                const nct_params* prm, const nct_seq_params* seq, const nct_seq_hold* hold);
int nct_seq_frame_multi_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* levels, const nct_seq_levels* seq_levels,
                               const nct_seq_hold_levels* hold_levels);
int nct_seq_frame_multi_stage_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* levels,
                                     const nct_color_stages* const* color, const nct_seq_levels* seq_levels, const nct_seq_hold_levels* hold_levels);
int nct_select_reference_hold(nct_ctx* ctx, const float* const* err, const uint8_t* const* guide_bgr, int K, int h, int w, const uint8_t* prev_label, const uint8_t* lab,
                              const uint8_t* lab_prev, const int16_t* field, double hold, double sigma, uint8_t* label, uint8_t* guide_out, float* err_out,
                              uint8_t* free_label, double* margin);
int nct_select_reference_hold_dev(nct_ctx* ctx, const float* const* d_err, const uint8_t* const* d_guide_bgr, int K, int h, int w, const uint8_t* d_prev_label,
                                  const uint8_t* d_lab, const uint8_t* d_lab_prev, const int16_t* d_field, double hold, double sigma, uint8_t* d_label, uint8_t* d_guide_out,
                                  float* d_err_out, uint8_t* d_free_label, double* d_margin);

/* ---- adaptive key frames (SPEC §6.7; an extension). Which frames of a sequence run the whole pair is decided per frame from how much of the frame the motion field
 * fails to explain, measured on the 8-bit Lab level images before any expensive stage runs.
 * nct_seq_change: the measure alone (rule 1), integers only. lab / lab_prev h*w*3 (8-bit Lab, the frame's and the previous frame's), field (nullable: m = 0) int16
 * [h*w][2] of (my, mx), a vector that leaves the grid first clamped component-wise so that p + m is inside. r(p) = sum over the three bytes of
 * |lab(p) - lab_prev(p + m(p))| (0 … 765); out->sad = sum_p r(p), out->changed = the number of pixels with r(p) > threshold, out->pixels = h * w. Host pointers,
 * synchronous; the _dev form takes device pointers (d_out: 16 bytes on the device) and is enqueued on the context's stream. NCT_ERR_INVALID with a message naming the
 * argument: a null image or a null out, a grid outside 1 … 4096 per side, a threshold outside [0, 765]. (The record's type is nct_seq_change_rec: C has one name space for
 * functions and typedef names.)
 * nct_seq_probe (rule 2): on an open sequence with state, the measure of the frame src_bgr against the previous frame at level lambda = min(levels - 1, 2) in run order
 * (0 = coarsest): the frame goes into scratch, its pyramid is built as a full frame builds it, L_t[l] is taken for l = 0 … lambda, with motion on the fields of §6.4 rules
 * 1-3 are found level by level against the kept packed maps (with motion off there is no field), then rule 1 with a->threshold. The probe reads the kept L and packed maps
 * and writes neither; X', the frame count and the counters below stay as they are; the per-level field buffers serve as scratch (every frame path rewrites them before it
 * reads them); everything else comes from the arena for the call and goes back. Synchronous. out: the decision this frame would get (rule 3), its counters not updated.
 * No open sequence, or one without state (the first frame after nct_seq_begin / nct_seq_reset): NCT_ERR_STATE; a null image or out, parameters out of range: NCT_ERR_INVALID.
 * The decision (rule 3), exact 64-bit integer comparisons in this order — NCT_SEQ_FIRST: the sequence has no state (no probe runs; change is zero, level -1);
 * NCT_SEQ_CUT: changed * 1000 >= cut_permille * pixels; NCT_SEQ_KEY: gap >= max_gap - 1, or key_permille != 1001 and (acc + changed) * 1000 >= key_permille * pixels; NCT_SEQ_PROPAGATED otherwise.
 * gap = the propagated frames since the last full frame, whichever call ran them; acc = the sum of `changed` over the frames nct_seq_frame_auto propagated since the last
 * full frame. nct_seq_begin, nct_seq_reset and every full frame (a manual nct_seq_frame too) zero both; a manual nct_seq_frame_propagate adds 1 to gap only.
 * threshold in [0, 765], cut_permille and key_permille in [0, 1001] (1001 = never), max_gap in [1, 1000]; anything else NCT_ERR_INVALID. a == NULL: the defaults.
 * nct_seq_decision: acc_changed and gap are the counters the rules compared against, before this frame's update; probe_ms the host wall time of the probe, its
 * synchronise included (0 for NCT_SEQ_FIRST). nct_pair_timing keeps its layout.
 * nct_seq_frame_auto (rule 4): probe, decide, then exactly one of the existing calls, unchanged — FIRST / KEY: nct_seq_frame; CUT: nct_seq_reset, then nct_seq_frame;
 * PROPAGATED: nct_seq_frame_propagate — and the update of acc and gap. timing (nullable) is the chosen call's, out (nullable) the decision. Every frame's bytes and the
 * state after it are those of the manual call the decision names; a CUT frame is nct_process_pair(S_t, R). key_permille = 0 with cut_permille = 1001 gives the all-full
 * sequence; cut_permille = key_permille = 1001 with max_gap = N gives the key-frame grid N. A refused call changes nothing; a frame that fails after the probe leaves the
 * sequence reset. A sequence that never calls these entry points keeps its bytes, its launches and its arena size. */
typedef struct nct_seq_change_rec { uint64_t sad; uint32_t changed, pixels; } nct_seq_change_rec;
typedef struct nct_seq_auto { int threshold, cut_permille, key_permille, max_gap; } nct_seq_auto;
void nct_seq_auto_default(nct_seq_auto* p);     /* 24, 500, 100, 8 */
enum { NCT_SEQ_FIRST = 0, NCT_SEQ_PROPAGATED = 1, NCT_SEQ_KEY = 2, NCT_SEQ_CUT = 3 };
typedef struct nct_seq_decision { int kind, level; nct_seq_change_rec change; uint32_t acc_changed; int gap; double probe_ms; } nct_seq_decision;
int nct_seq_change(nct_ctx* ctx, const uint8_t* lab, const uint8_t* lab_prev, int h, int w, const int16_t* field, int threshold, nct_seq_change_rec* out);
int nct_seq_change_dev(nct_ctx* ctx, const uint8_t* d_lab, const uint8_t* d_lab_prev, int h, int w, const int16_t* d_field, int threshold, nct_seq_change_rec* d_out);
int nct_seq_probe(nct_ctx* ctx, const uint8_t* src_bgr, const nct_seq_auto* a, nct_seq_decision* out);
int nct_seq_frame_auto(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_auto* a, nct_seq_decision* out);

/* ---- 3D colour look-up tables (SPEC §6.6; an extension: the reference leaves every result as pixels). A table hands a computed look to other tools (.cube) and puts it on
 * pixels the pyramid never saw: a photograph above the working size, the frames of a clip. Lattice size N in {3, 5, 9, 17, 33, 65}; a table is float [N][N][N][3] indexed
 * [ib][ig][ir], channels BGR, values in grey levels, not clamped.
 * nct_lut_fit: from two images of npix pixels each, a source S and a result O (8-bit BGR, tightly packed). (1) splat: per lattice node the integer sums W = sum w and
 * R[c] = sum w (O_c - S_c) over all pixels, w the pixel's trilinear integer weight (eight per pixel, summing to 255^3); (2) solve: the displacement field D (double) that
 * minimises sum_n W_n / 255^3 (D_n - R_n / W_n)^2 + lambda sum_edges (D_u - D_v)^2 over the lattice's 6-neighbour edges, by a fixed number of multigrid cycles: empty
 * cells are filled by the smoothness term; (3) LUT_n[c] = (float)(node colour_c + D_n[c]). stages (nullable, its arrays nullable) receives W [N^3], R [N^3][3], D [N^3][3].
 * nct_lut_apply: out_c = saturate_cast<uchar>(sum over the eight corners of w LUT[c] / 255^3), the sum in double; the table whose nodes are the node colours returns the
 * input. out_bgr may be bgr. The host form refuses a table with a non-finite entry; the _dev form does not look.
 * The _dev forms take device pointers (stages: a host struct of device pointers) and are enqueued on the context's stream like the other device-pointer seams.
 * nct_pair_fit_lut: the fit from the source and the result the context's last finished run holds on the device (nct_pair_run, nct_multi_run, nct_seq_frame and what is built
 * on them: at the result's size; nct_process_pair_fullres: the original source and the full-resolution result), no PCIe round trip but the table's; synchronous. Without a
 * finished run: NCT_ERR_STATE.
 * NCT_ERR_INVALID with a message: a size outside the set, a lambda that is not finite and greater than 0, a null pointer, npix < 1 or npix > 2^26. */
typedef struct nct_lut_params { int size; double lambda; } nct_lut_params;
void nct_lut_params_default(nct_lut_params* p);     /* size 33, lambda 0.1 (the sweep) */
typedef struct nct_lut_stages { uint64_t* weight; int64_t* resid; double* disp; } nct_lut_stages;
int nct_lut_fit(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, size_t npix, const nct_lut_params* prm, float* lut_out, nct_lut_stages* stages);
int nct_lut_fit_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, size_t npix, const nct_lut_params* prm, float* d_lut_out, nct_lut_stages* d_stages);
int nct_lut_apply(nct_ctx* ctx, const float* lut, int size, const uint8_t* bgr, size_t npix, uint8_t* out_bgr);
int nct_lut_apply_dev(nct_ctx* ctx, const float* d_lut, int size, const uint8_t* d_bgr, size_t npix, uint8_t* d_out_bgr);
int nct_pair_fit_lut(nct_ctx* ctx, const nct_lut_params* prm, float* lut_out);

/* ---- shot look-up tables and the 16-bit apply (SPEC §6.20; an extension of §6.6). One table for a whole shot, fitted over many frames, and a table put onto originals
 * deeper than 8 bits. C ABI and python binding only: no console option.
 * nct_lut_apply_u16: the table of §6.6 on 16-bit pixels ([npix][3] uint16 BGR, tightly packed), a value v standing for the grey level v / 257. Per axis t = v (N - 1),
 * i = min(t / 65535, N - 2), f = t - 65535 i, integer weights (65535 - f, f); out_c = the sum over the eight corners of w LUT[c] in double, / 65535^3, * 257, clamped to
 * [0, 65535] (a NaN becomes 0) and rounded to nearest even. The identity table returns every input; on 257 u the result is within half a 16-bit step plus half an 8-bit
 * one of 257 times nct_lut_apply's on u. out_bgr16 may be bgr16. The host form refuses a table with a non-finite entry; the _dev form does not look. Refusals as
 * nct_lut_apply's.
 * nct_lut_accum_*: one accumulator per context, owned by it from begin to end (device blocks, zeroed at begin), independent of pairs and sequences: it survives
 * nct_pair_upload, every run, nct_seq_begin / _end / _reset, and goes with nct_destroy. After the adds (S_1, O_1, M_1) ... (S_k, O_k, M_k) its W and R are §6.6 rule 3's
 * sums over all offered pixels with M >= 128 (mask NULL: every pixel), so nct_lut_accum_solve(lambda) — rules 4-8 on them — gives the table, and in stages W, R and D,
 * of nct_lut_fit_masked on the arrays laid end to end, bit for bit, in any order of the adds. An add is one splat launch; one whose mask keeps no pixel changes neither
 * the sums nor pixels_kept. add_dev is enqueued on the context's stream and does not wait. add_run offers the images nct_pair_fit_lut would read after the context's last
 * finished run (its mask included), from where they lie on the device; without a finished run: NCT_ERR_STATE, nothing changes. solve does not consume: more adds and
 * another solve give the fit over everything so far. With nothing kept solve returns NCT_ERR_INVALID; solve_dev waits for that one number (only when a masked add
 * was made) before it enqueues. info: pointers nullable; it waits for the stream where pixels_kept is asked for and a masked add was made.
 * Limits: 1 <= npix <= 2^26 per add, at most 2^30 pixels offered between begin and end (R stays below 2^62, W below 2^54): the add that would pass it is refused with
 * NCT_ERR_INVALID from the host-side count, before anything is enqueued. begin while one is open, and every other call without one: NCT_ERR_STATE. A size outside the
 * set, a lambda that is not finite and greater than 0, a null src / res / lut_out: NCT_ERR_INVALID. */
int nct_lut_apply_u16(nct_ctx* ctx, const float* lut, int size, const uint16_t* bgr16, size_t npix, uint16_t* out_bgr16);
int nct_lut_apply_u16_dev(nct_ctx* ctx, const float* d_lut, int size, const uint16_t* d_bgr16, size_t npix, uint16_t* d_out_bgr16);
int nct_lut_accum_begin(nct_ctx* ctx, int size);
int nct_lut_accum_add(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, const uint8_t* mask /* nullable */, size_t npix);
int nct_lut_accum_add_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, const uint8_t* d_mask /* nullable */, size_t npix);
int nct_lut_accum_add_run(nct_ctx* ctx);
int nct_lut_accum_info(nct_ctx* ctx, int* size, uint64_t* adds, uint64_t* pixels_offered, uint64_t* pixels_kept);
int nct_lut_accum_solve(nct_ctx* ctx, double lambda, float* lut_out, nct_lut_stages* stages);
int nct_lut_accum_solve_dev(nct_ctx* ctx, double lambda, float* d_lut_out, nct_lut_stages* d_stages);
int nct_lut_accum_end(nct_ctx* ctx);

/* ---- local colour grids (SPEC §6.22; an extension): the spatial counterpart of the table — a bilateral grid of affine colour maps (Chen et al., Bilateral Guided
 * Upsampling; HDRnet's slicing layer). A grid is double[gy][gx][gz][3][4] over (row, column, luma), gy, gx in [2, 64], gz in [2, 32]; a node holds a 3 x 4 map of BGR
 * as a DISPLACEMENT in grey levels, output channel c in B, G, R, input term j in B, G, R, 1: out_c = s_c + X_c . (s_B, s_G, s_R, 1). The all-zero grid is the identity.
 * It works in BGR grey levels throughout: no Lab conversion. Positions depend on relative position only (row y of h: t = (2y + 1)(gy - 1) over 2h; luma
 * Y = (29 B + 150 G + 77 R + 128) >> 8: t = Y (gz - 1) over 255 or 65535), so a grid fitted at one size applies to any picture of the same framing.
 * nct_grid_fit: from two 8-bit images of h x w pixels, a source S and a result O (BGR, tightly packed). (1) splat: per node, over the pixels whose NEAREST node it
 * is, the 22 int64 sums — the 10 distinct sums s_j s_k over (B, G, R, 1), [9] the count, then the 12 sums s_j (O_c - S_c), [10 + 4c + j]; (2) one integer [1 2 1]
 * pass along each axis, out-of-grid taps dropped; (3) per node with a count, the 4 x 4 system (blurred Gram matrix, lambda * count added to the three linear
 * diagonal entries) solved by L D L^T for the three channels; a node without a count gets 0. stages (nullable, its arrays nullable) receives the sums of (1) and (2),
 * [gy*gx*gz][22] each. lambda is finite and in [1/16, 65536].
 * nct_grid_apply / nct_grid_apply_u16: per pixel the eight corner weights as integers, the 12 coefficients interpolated in double in a fixed order,
 * v = s_c + (((a_0 B + a_1 G) + a_2 R) + a_3 K) / (2h * 2w * Z), K = 1 and Z = 255 for 8 bits, K = 257 and Z = 65535 for 16 bits (a value v standing for the grey
 * level v / 257), clamped to [0, Z] (a NaN becomes 0) and rounded to nearest even. out may be the input. The host forms refuse a grid with a non-finite entry; the
 * _dev forms do not look. Host forms are synchronous, _dev forms are enqueued on the context's stream.
 * nct_pair_fit_grid: the fit from the images nct_pair_fit_lut would read after the context's last finished run; a run's mask is not read (kept pixels fit a zero
 * displacement). Without a finished run: NCT_ERR_STATE.
 * A null pointer, h or w outside [1, 16384], more than 2^26 pixels, a node count out of range, a bad lambda: NCT_ERR_INVALID with a message naming the argument. */
typedef struct nct_grid_params { int gy, gx, gz; double lambda; } nct_grid_params;
void nct_grid_params_default(nct_grid_params* p);   /* 16, 16, 16, lambda 16 */
typedef struct nct_grid_stages { int64_t* sums; int64_t* blurred; } nct_grid_stages;
int nct_grid_fit(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, int h, int w, const nct_grid_params* prm, double* grid_out, nct_grid_stages* stages);
int nct_grid_fit_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, int h, int w, const nct_grid_params* prm, double* d_grid_out, nct_grid_stages* d_stages);
int nct_grid_apply(nct_ctx* ctx, const double* grid, int gy, int gx, int gz, const uint8_t* bgr, int h, int w, uint8_t* out_bgr);
int nct_grid_apply_dev(nct_ctx* ctx, const double* d_grid, int gy, int gx, int gz, const uint8_t* d_bgr, int h, int w, uint8_t* d_out_bgr);
int nct_grid_apply_u16(nct_ctx* ctx, const double* grid, int gy, int gx, int gz, const uint16_t* bgr16, int h, int w, uint16_t* out_bgr16);
int nct_grid_apply_u16_dev(nct_ctx* ctx, const double* d_grid, int gy, int gx, int gz, const uint16_t* d_bgr16, int h, int w, uint16_t* d_out_bgr16);
int nct_pair_fit_grid(nct_ctx* ctx, const nct_grid_params* prm, double* grid_out);

/* ---- source region masks (SPEC §6.11; an extension): recolour only part of the source. A mask M has one byte per SOURCE pixel: 0 keeps the source, 255 is the full
 * transfer, values between are partial. The level masks are the single-channel form of the image pyramid: M_top = M at the working size, M_l = nct_resize_u8c1 of
 * M_(l+1) to level l's grid; nct_resize_u8c1 is channel 0 of nct_resize_u8c3 on (M, M, M), the INTER_AREA switch included. Every level of a masked run has two steps
 * more than nct_pair_run's: between S1 and U1 the mix moves S1's coefficients toward the identity transform, with m = M_l(p) / 255 in double a' = 1 + m (a - 1),
 * b' = m b (M_l = 255: the six 64-bit words are copied, a NaN stays that NaN; M_l = 0: a = 1, b = 0, which heals a NaN), and X' replaces S1's output in U1, roughness,
 * S2 and A1 — S2's edge-aware smoothing then carries the transition along the source's own edges; behind A1 the compose, at the size the finish targets with the mask at
 * that size, writes out(p) = keep ? S(p) : Lab2BGR(Lab_o(p)), keep = (protect and M(p) == 0) or (M(p) != 255 and Lab_o(p) == nct_bgr2lab_u8(S)(p) on all three bytes):
 * a pixel whose Lab value did not move keeps its source bytes instead of the Lab round trip's. The composed image is the level's result and what the next level's
 * re-predict reads. protect (default 0) trades a possible step at a binary mask drawn through a smooth region for the guarantee that an M == 0 pixel never changes.
 * No mask: today's bytes, launches and arena. M == 255 everywhere: nct_process_pair's bytes. M == 0 everywhere: the source, byte for byte.
 * nct_resize_u8c1, nct_region_mix (x, x_out [2][h*w][3], mask h*w; grid sides 1 … 4096), nct_region_compose (s_bgr, lab_out, out_bgr npix*3, mask npix; 1 <= npix <= 2^26;
 * Lab -> BGR in the form prm->flags selects): the three steps alone on host pointers, synchronous; the _dev forms take device pointers and are enqueued on the context's
 * stream (nct_region_mix_dev: x_out may be x; nct_region_compose_dev converts S to Lab in an arena block that goes back in stream order).
 * nct_pair_set_region: after nct_pair_upload / nct_multi_upload, copies the mask (sh x sw of the uploaded source) to the device; nct_pair_run, nct_multi_run and their
 * _levels forms then run masked, nct_pair_fit_lut fits over the pixels with M >= 128 (the mask at the size it reads). NULL removes the mask; the next upload drops it.
 * No uploaded source, or an open sequence: NCT_ERR_STATE (sequences with a mask are not defined). region NULL: the defaults; protect outside {0, 1}: NCT_ERR_INVALID.
 * nct_pair_run_region_levels: nct_pair_run_levels (levels nullable) plus, per level, the level mask and X' — color[l]->ab_nonlocal stays S1's output BEFORE the mix,
 * ab_up / roughness / ab_wls come after it. With region levels asked for and no mask set: NCT_ERR_STATE. The mix's time counts in nct_pair_timing.color_ms.
 * nct_process_pair_region = nct_pair_upload + nct_pair_set_region + nct_pair_run + nct_pair_download; mask NULL: nct_process_pair.
 * nct_process_pair_fullres_region: nct_process_pair_fullres with a mask at the ORIGINAL size: the working mask is nct_resize_u8c1 of mask0 to nct_working_size's size, the
 * last level mixes on its grid with the working-size level mask and composes at sh x sw with mask0; a source that is not shrunk gives nct_process_pair_region's bytes;
 * nct_pair_fit_lut afterwards uses mask0. nct_process_pair_fullres_finish_region: the same with the finish chosen; NCT_FINISH_UPSAMPLE (plain or guided) with a mask is
 * not defined and refused with NCT_ERR_INVALID. mask0 NULL: nct_process_pair_fullres_finish.
 * nct_lut_fit_masked[_dev]: nct_lut_fit whose splat skips the pixels with mask < 128 — the fit of the subsequence of kept pixels; mask NULL: nct_lut_fit. A mask that
 * keeps no pixel: NCT_ERR_INVALID. The masked _dev form waits for its splat (it has to learn whether a pixel was kept) before it enqueues the solve.
 * A mask on the REFERENCE ("take colours only from the sky"): the next block (SPEC §6.12). */
typedef struct nct_region_params { int protect; } nct_region_params;
void nct_region_params_default(nct_region_params* p);     /* protect 0 */
typedef struct nct_region_levels { double* ab_mix[5]; uint8_t* mask[5]; } nct_region_levels;   /* X' [2][h*w][3]; M_l [h*w]; all nullable */
int nct_resize_u8c1(nct_ctx* ctx, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);
int nct_resize_u8c1_dev(nct_ctx* ctx, const uint8_t* d_src, int sh, int sw, uint8_t* d_dst, int dh, int dw);
int nct_region_mix(nct_ctx* ctx, const double* x, const uint8_t* mask, int h, int w, double* x_out);
int nct_region_mix_dev(nct_ctx* ctx, const double* d_x, const uint8_t* d_mask, int h, int w, double* d_x_out);
int nct_region_compose(nct_ctx* ctx, const uint8_t* s_bgr, const uint8_t* lab_out, const uint8_t* mask, size_t npix, const nct_region_params* region, const nct_params* prm,
                       uint8_t* out_bgr);
int nct_region_compose_dev(nct_ctx* ctx, const uint8_t* d_s_bgr, const uint8_t* d_lab_out, const uint8_t* d_mask, size_t npix, const nct_region_params* region,
                           const nct_params* prm, uint8_t* d_out_bgr);
int nct_pair_set_region(nct_ctx* ctx, const uint8_t* mask, const nct_region_params* region);
int nct_pair_run_region_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_region_levels* region_levels);
int nct_process_pair_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask, const uint8_t* ref_bgr, int rh, int rw, const nct_region_params* region,
                            const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing);
int nct_process_pair_fullres_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, int max_side,
                                    const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr /* sh x sw x 3 */, nct_pair_timing* timing);
int nct_process_pair_fullres_finish_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, int max_side,
                                           int finish, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr /* sh x sw x 3 */, nct_pair_timing* timing);
int nct_lut_fit_masked(nct_ctx* ctx, const uint8_t* src_bgr, const uint8_t* res_bgr, const uint8_t* mask, size_t npix, const nct_lut_params* prm, float* lut_out,
                       nct_lut_stages* stages);
int nct_lut_fit_masked_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, const uint8_t* d_res_bgr, const uint8_t* d_mask, size_t npix, const nct_lut_params* prm, float* d_lut_out,
                           nct_lut_stages* d_stages);

/* ---- reference region masks (SPEC §6.12; an extension): take colours from part of the reference. A mask Q_k has one byte per pixel of REFERENCE k: 0 = excluded,
 * 255 = allowed, between = partial. The votes are not masked — the mask is voted: Q_k's pyramid (Q_k,top = Q_k, Q_k,l = nct_resize_u8c1 of Q_k,(l+1) onto the
 * reference's level grid) is carried to the source through the level's NNFs by B1's taps, bounds tests and source lists, P_k,l(p) = (uint8) rint((A wa + B wb) /
 * (ca wa + cb wb)) in double (A, ca: coherence sum and count over the nine taps of ann; B, cb: completeness sum and count over bnn's sources; wa = w_coherence / (ah aw),
 * wb = w_complete / (bh bw)): nct_bds_vote_image on one channel, rounded to nearest where that truncates, so that Q == 255 gives exactly 255 and Q == 0 exactly 0. With
 * several references P_l(p) = P_label(p),l(p) (a reference without a mask: 255). The level mask M_l = min(P_l, the source's level mask of §6.11 or 255) drives §6.11's
 * mix; the target mask F_l = nct_resize_u8c1(P_l -> the size the level's finish targets), then the minimum with the source mask at that size, drives §6.11's compose with
 * the run's protect. A source pixel whose correspondences land in the excluded part keeps its colours; it is not forced onto the allowed part, and where P is partial the
 * guidance colour is still B1's vote over allowed and excluded pixels alike: only the strength of the transfer follows the mask. No reference mask: today's bytes, launches
 * and arena. Every Q_k == 255: nct_process_pair's / nct_process_multi's bytes (with a source mask: nct_process_pair_region's). K = 1 and Q == 0: the source, byte for byte.
 * nct_region_pull: the pull alone on host pointers, synchronous (q_mask bh x bw, ann ah x aw words, bnn bh x bw words, out ah x aw bytes; grid sides 1 … 4096; a null
 * pointer or a side out of range: NCT_ERR_INVALID, the message names the argument); nct_region_pull_dev: device pointers, enqueued on the context's stream.
 * nct_pair_set_ref_region: after nct_pair_upload / nct_multi_upload, copies reference k's mask (rh[k] x rw[k] of the uploaded reference); nct_pair_run, nct_multi_run and
 * their _levels forms then run masked, nct_pair_fit_lut fits over the pixels whose last level's F is >= 128. mask NULL removes reference k's; the next upload drops all.
 * k outside [0, K) or protect outside {0, 1}: NCT_ERR_INVALID; no upload, or an open sequence: NCT_ERR_STATE (a sequence takes its reference masks through nct_seq_set_ref_region, SPEC §6.19). region non-NULL
 * sets the run's protect — the last setter called decides it, nct_pair_set_region or this one; region NULL leaves it.
 * nct_multi_run_ref_region_levels: nct_multi_run_levels (levels nullable) plus per level Q_k,l [bh*bw], P_k,l [h*w] (masked references only), M_l [h*w], F_l [H*W] and X'
 * [2][h*w][3]; with no reference mask set: NCT_ERR_STATE. nct_pair_run_ref_region_levels: the same for a pair, beside nct_pair_run_levels' maps (the colour stages included).
 * Scratch: while a pull runs it holds 144 bytes per REFERENCE pixel of the level from the context's arena (two arrays of nine 64-bit words, plus the scan's own and the
 * inverse map's 20): 70 MB at 700 x 700, 2.3 GB at 4000 x 4000, 2.4 GB at nct_region_pull's largest grid; a device that cannot give it answers NCT_ERR_HIP. The pull and the merge count in nct_pair_timing.vote_ms / vote_level_ms, the mix in color_ms.
 * nct_process_pair_ref_region = upload + nct_pair_set_region (src_mask non-NULL) + nct_pair_set_ref_region (ref_mask non-NULL) + run + download; both NULL:
 * nct_process_pair. nct_process_multi_ref_region: the same for K references, ref_masks and each of its K entries nullable. nct_process_pair_fullres_ref_region: both masks
 * at the ORIGINAL sizes, shrunk with their images by nct_resize_u8c1; the exact finish only: the last level resizes its P to sh x sw, takes the minimum with mask0 where
 * set and composes on the original; a source that is not shrunk gives nct_process_pair_ref_region's bytes. No entry point takes a reference mask and the upsampling finish.
 * Restricting PatchMatch's candidates to the allowed region is a different feature and not part of this. */
typedef struct nct_ref_region_levels {
    uint8_t* ref_mask[NCT_MAX_REFS][5];    /* Q_k,l */
    uint8_t* pulled[NCT_MAX_REFS][5];      /* P_k,l */
    uint8_t* mask[5];                      /* M_l */
    uint8_t* mask_full[5];                 /* F_l */
    double* ab_mix[5];                     /* X' */
} nct_ref_region_levels;                   /* all nullable */
int nct_region_pull(nct_ctx* ctx, const uint8_t* q_mask, int bh, int bw, const uint32_t* ann, const uint32_t* bnn, int ah, int aw, double w_coherence, double w_complete,
                    uint8_t* out);
int nct_region_pull_dev(nct_ctx* ctx, const uint8_t* d_q_mask, int bh, int bw, const uint32_t* d_ann, const uint32_t* d_bnn, int ah, int aw, double w_coherence,
                        double w_complete, uint8_t* d_out);
int nct_pair_set_ref_region(nct_ctx* ctx, int k, const uint8_t* mask, const nct_region_params* region);
int nct_multi_run_ref_region_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_multi_levels* levels, const nct_ref_region_levels* region_levels);
int nct_pair_run_ref_region_levels(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_ref_region_levels* region_levels);
int nct_process_pair_ref_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* src_mask, const uint8_t* ref_bgr, int rh, int rw, const uint8_t* ref_mask,
                                const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing);
int nct_process_multi_ref_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* src_mask, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw,
                                 const uint8_t* const* ref_masks, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr, nct_pair_timing* timing);
int nct_process_pair_fullres_ref_region(nct_ctx* ctx, const uint8_t* src_bgr, int sh, int sw, const uint8_t* mask0, const uint8_t* ref_bgr, int rh, int rw, const uint8_t* ref_mask0,
                                        int max_side, const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr /* sh x sw x 3 */, nct_pair_timing* timing);

/* ---- region masks in sequences (SPEC §6.13; an extension): §6.11's source mask on the frames of an open sequence, and the masked upsampling finish.
 * nct_seq_set_region: on an open sequence, between frames. mask has one byte per pixel at the size frames arrive — sh x sw after nct_seq_begin, the original size after
 * nct_seq_begin_fullres, where it is also shrunk on the device to the working size by nct_resize_u8c1 — and is copied to the device in the call. It is sticky: every later
 * nct_seq_frame, _levels, _propagate, _propagate_levels and nct_seq_frame_auto runs masked until the mask is replaced or removed with mask == NULL; nct_seq_reset keeps
 * it, nct_seq_end and nct_destroy drop it. region NULL: the defaults. No open sequence: NCT_ERR_STATE; protect outside {0, 1}: NCT_ERR_INVALID, and the setting stays as
 * it was. A caller with a matte per frame calls it before every frame.
 * A full frame runs per level S1, §6.3's blend (into the kept state, unchanged), §6.11's mix OUT OF PLACE from the kept X'_t into the level's own map, U1 / roughness /
 * S2 / A1 on the mixed map, §6.11's compose. The kept X' is never mixed: a matte that moves or changes needs no reset, and the next frame's blend never sees this frame's
 * matte. A propagated frame runs §6.5 unchanged on the unmixed state, then mixes the top level run's X'_t with that level's mask into 48 B per level pixel of scratch and
 * finishes on that; only the level masks down to the top level run are built. Finishes: the working size and NCT_FINISH_EXACT compose as §6.11 rules 3 and 5; with
 * NCT_FINISH_UPSAMPLE (plain or guided) the working-size finish runs as in a working-size masked sequence and the masked upsampling finish follows: per original pixel
 * Lab_S and Lab_o as nct_color_finish_upsample / nct_color_finish_guided compute them up to A1, keep = (protect and M0 == 0) or (M0 != 255 and Lab_o == Lab_S on all
 * three bytes), out = keep ? S0 : Lab2BGR(Lab_o). One kernel, 3 + 1 B read and 3 B written per original pixel, no original-size intermediate.
 * No nct_seq_set_region call: the sequence's bytes, launches and arena of before. M == 255: the unmasked sequence's bytes and state; M == 0: every frame is its source.
 * A first frame, a frame after nct_seq_reset, a CUT frame and every frame with tau == 0 equal nct_process_pair_region (NCT_FINISH_EXACT: nct_process_pair_fullres_region).
 * nct_seq_probe's record and nct_seq_frame_auto's decisions do not depend on the mask. nct_pair_fit_lut after a masked frame fits over M >= 128 at the size it reads.
 * nct_seq_frame_region_levels / nct_seq_frame_propagate_region_levels: the _levels forms plus nct_region_levels — ab_mix[l] = the mixed map the finish read (a propagated
 * frame: the top level run only), mask[l] = M_l; seq_levels->ab_blend[l] stays the unmixed kept state. Region levels asked for and no mask set: NCT_ERR_STATE.
 * nct_color_finish_upsample_region[_dev], nct_color_finish_guided_region[_dev]: the masked upsampling finish alone; the arguments, limits and refusals of the unmasked
 * calls plus mask (H*W bytes; NULL: the unmasked call) and region (NULL: the defaults; a bad protect: NCT_ERR_INVALID). Equal sizes keep the copy path.
 * Reference masks in sequences: SPEC §6.19 below (nct_pair_set_ref_region keeps its refusal). Not defined: a masked upsampling finish for
 * pairs through nct_process_pair_fullres_finish_region (its refusal stays; a one-frame full-resolution sequence gives those bytes). */
int nct_seq_set_region(nct_ctx* ctx, const uint8_t* mask, const nct_region_params* region);
int nct_seq_frame_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_seq_levels* seq_levels,
                                const nct_region_levels* region_levels);
int nct_seq_frame_propagate_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels,
                                          const nct_region_levels* region_levels);
int nct_color_finish_upsample_region(nct_ctx* ctx, const double* ab_wls, int h, int w, const uint8_t* s_bgr_full, int H, int W, const uint8_t* mask /* H*W */,
                                     const nct_region_params* region, const nct_params* prm, uint8_t* out_bgr_full);
int nct_color_finish_upsample_region_dev(nct_ctx* ctx, const double* d_ab_wls, int h, int w, const uint8_t* d_s_bgr_full, int H, int W, const uint8_t* d_mask /* H*W */,
                                         const nct_region_params* region, const nct_params* prm, uint8_t* d_out_bgr_full);
int nct_color_finish_guided_region(nct_ctx* ctx, const double* ab_wls, const uint8_t* lab_work, int h, int w, const uint8_t* s_bgr_full, int H, int W, const uint8_t* mask /* H*W */,
                                   const nct_region_params* region, const nct_guided_params* guided, const nct_params* prm, uint8_t* out_bgr_full);
int nct_color_finish_guided_region_dev(nct_ctx* ctx, const double* d_ab_wls, const uint8_t* d_lab_work, int h, int w, const uint8_t* d_s_bgr_full, int H, int W,
                                       const uint8_t* d_mask /* H*W */, const nct_region_params* region, const nct_guided_params* guided, const nct_params* prm,
                                       uint8_t* d_out_bgr_full);

/* ---- reference region masks in sequences (SPEC §6.19; an extension): §6.12's reference mask on the frames of an open sequence — pulled on full frames, held with the
 * blend's own weight, carried on propagated frames. C ABI and python only: the console driver has no option for it.
 * nct_seq_set_ref_region: on an open sequence (plain, multi or full-resolution), between frames. mask has one byte per pixel of reference k at the size that reference
 * arrived — in a full-resolution sequence the original size, shrunk on the device by nct_resize_u8c1 to the reference's working size — and is copied in the call; its
 * level masks Q_k,l (§6.12 rule 1) are built once, here, and kept. Sticky until replaced or removed (mask NULL); nct_seq_reset keeps it, nct_seq_end and nct_destroy drop
 * it. region non-NULL sets the run's protect (the last setter called decides it); NULL leaves it. No open sequence: NCT_ERR_STATE; k outside [0, K) or protect outside
 * {0, 1}: NCT_ERR_INVALID, and the setting stays as it was. nct_pair_set_ref_region keeps its NCT_ERR_STATE while a sequence is open.
 * A full frame, per level l: §6.12 rule 2's pull per masked reference behind its votes; §6.12 rule 3's merge with the level's label map (§6.18's l_t with K > 1) gives P_l;
 * then the hold, on a frame that blends (the sequence has state, tau > 0, and a kept P'_(t-1)[l] exists), per level pixel p in IEEE double, uncontracted:
 *   m(p) = the level's field as in §6.18 rule 2, clamped so that p + m is inside the grid, 0 with motion off; j = P'_(t-1)[l](p + m(p));
 *   tau_p = the weight §6.3 rule 3 (§6.4 rule 4 with a field) gives the pixel, the value nct_seq_levels.tau_map reports;
 *   P'_t(p) = (uint8) rint((double)P_l(p) + tau_p * ((double)j - (double)P_l(p))).
 * On every other full frame — a first frame, a frame after nct_seq_reset or a cut, tau == 0, the first full frame after any set, replace or remove of a reference mask —
 * P'_t = P_l with no launch. P'_t replaces the kept map out of place. M_l = min(P'_t, the source level mask in force or 255) drives §6.13 rule 2's out-of-place mix (the
 * kept X' is never mixed), F_l = nct_resize_u8c1(P'_t -> the size the level's finish targets) then the minimum with the source mask at that size drives the compose with
 * the run's protect. The last level's finish follows the sequence's form: the working size; NCT_FINISH_EXACT with F at the original size; NCT_FINISH_UPSAMPLE (plain or
 * guided) composes at the working size and runs the masked upsampling finish with F0 = min(resize(P'_top -> H0 x W0), M0), 1 B per original pixel of scratch.
 * A propagated frame carries the kept map per level run, P'_t[l](p) = P'_(t-1)[l](p + m(p)) (bytes copied, never interpolated; left as they are with motion off), then
 * mixes, composes and finishes on the top level run only as §6.13 rule 3 does. While a reference mask is set and no kept P' exists — before the first full frame, or right
 * after a set, replace or remove — a propagated frame is NCT_ERR_STATE (a full frame must come first) and changes nothing, and nct_seq_frame_auto turns a PROPAGATED
 * decision into KEY and reports KEY; nct_seq_probe is unchanged. No nct_seq_set_ref_region call: the sequence's bytes, kept state, launches and arena of before. Every
 * Q_k == 255: the unmasked sequence's bytes and state. K = 1, Q == 0: every frame is its source. A first frame, a frame after reset, a CUT frame and every frame with
 * tau == 0 equal nct_process_pair_ref_region / nct_process_multi_ref_region (NCT_FINISH_EXACT: nct_process_pair_fullres_ref_region). nct_pair_fit_lut after such a frame
 * fits over the last level's F >= 128 at the size it reads.
 * Arena while a reference mask is set: 2 x 1 B per level pixel of every level run (P' and the map the gather writes), 1 B per reference level pixel per masked
 * reference, and §6.12's 144 B per reference pixel of the level during a pull.
 * nct_seq_pull_hold: the merge, the hold and the minimum alone on host maps (synchronous). pulled: K host pointers to h*w bytes (a null entry: 255); label h*w (nullable
 * when K == 1); prev h*w; lab / lab_prev h*w*3 (8-bit Lab); field (nullable: m = 0) int16 [h*w][2]; src_mask h*w (nullable: 255); p_out h*w; m_out and p_free (the merged
 * P_l before the hold) h*w, nullable. The _dev form takes device pointers (the array OF pointers is host memory), is enqueued on the context's stream and refuses a p_out
 * that overlaps prev. Grid sides outside 1 … 4096, K outside [1, NCT_MAX_REFS], tau outside [0, 1), sigma not finite and positive, a null input: NCT_ERR_INVALID, the
 * message names the argument.
 * nct_seq_frame_ref_region_levels: nct_seq_frame_multi_stage_levels plus nct_ref_region_levels (ref_mask = Q_k,l, pulled = P_k,l, mask = M_l, mask_full = F_l, ab_mix) and
 * nct_seq_pull_levels (p_free[l] = P_l, p_held[l] = P'_t; on a frame without a hold they are equal). nct_seq_frame_propagate_ref_region_levels: the propagated form; p_held
 * for every level run, the rest for the top level run only (p_free, pulled and ref_mask are not written). Either report asked for with no reference mask set: NCT_ERR_STATE. */
typedef struct nct_seq_pull_levels { uint8_t* p_free[5]; uint8_t* p_held[5]; } nct_seq_pull_levels;   /* all nullable */
int nct_seq_set_ref_region(nct_ctx* ctx, int k, const uint8_t* mask, const nct_region_params* region);
int nct_seq_pull_hold(nct_ctx* ctx, const uint8_t* const* pulled, int K, const uint8_t* label, const uint8_t* prev, const uint8_t* lab, const uint8_t* lab_prev,
                      const int16_t* field, const uint8_t* src_mask, int h, int w, double tau, double sigma, uint8_t* p_out, uint8_t* m_out, uint8_t* p_free);
int nct_seq_pull_hold_dev(nct_ctx* ctx, const uint8_t* const* d_pulled, int K, const uint8_t* d_label, const uint8_t* d_prev, const uint8_t* d_lab, const uint8_t* d_lab_prev,
                          const int16_t* d_field, const uint8_t* d_src_mask, int h, int w, double tau, double sigma, uint8_t* d_p_out, uint8_t* d_m_out, uint8_t* d_p_free);
int nct_seq_frame_ref_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* levels,
                                    const nct_color_stages* const* color, const nct_seq_levels* seq_levels, const nct_seq_hold_levels* hold_levels,
                                    const nct_ref_region_levels* region_levels, const nct_seq_pull_levels* pull_levels);
int nct_seq_frame_propagate_ref_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels,
                                              const nct_ref_region_levels* region_levels, const nct_seq_pull_levels* pull_levels);

/* ---- region tracking (SPEC §6.14; an extension): the matte of §6.13 follows the motion field of §6.4, so that it is drawn on one frame and carried through the shot.
 * nct_seq_matte_warp[_dev]: the carry alone. mask_prev: H x W bytes; field: h x w int16 pairs (my, mx), a backward field on a level grid (it points from the frame
 * into the previous one), 1 <= h <= H <= 16384, 1 <= w <= W <= 16384, h, w <= 4096, H * W <= 2^26. Per target pixel and axis (y shown): num = (2y + 1) h - H,
 * s = floor(num / 2H), t = num - 2H s, clamped to the grid with t = 0 at its ends, s1 = min(s + 1, h - 1) — nct_resize's centre-aligned index rule as an exact
 * fraction; the four vectors around (sy, sx) are weighted with (2H - ty, ty) x (2W - tx, tx) into the sum S, and d_y = floor((2 S_y H + den) / (2 den)),
 * den = h * 2H * 2W (d_x: W and w): the vector in target pixels, rounded half up. mask_out(y, x) = mask_prev(clamp(y + d_y, 0, H - 1), clamp(x + d_x, 0, W - 1)).
 * 64-bit integers only; a byte is copied, never interpolated: a binary matte stays binary, all-255 stays all-255, a zero field returns the input, and with H == h,
 * W == w this is nct_seq_warp's gather on bytes. The host form is synchronous; the _dev form is enqueued on the context's stream and refuses a mask_out that overlaps
 * mask_prev. A null pointer, a side out of range and a target smaller than the field grid are NCT_ERR_INVALID, the message names the argument.
 * nct_seq_set_region_tracking: on an open sequence, between frames; off (0) is the default, no open sequence is NCT_ERR_STATE, `on` outside {0, 1} NCT_ERR_INVALID.
 * A matte given to nct_seq_set_region belongs to the next frame that runs: that frame uses it as it came (age 0); a refused call and nct_seq_probe do not use it up.
 * While tracking is on, every later nct_seq_frame, _levels, _region_levels, _propagate* and nct_seq_frame_auto first carries the matte: M_t = matte_warp(M_(t-1), the
 * field of the frame's top level run against the previous frame), at the size frames arrive — a full-resolution sequence carries M0 at the original size with the
 * working-size level's field and shrinks the result with nct_resize_u8c1, as nct_seq_set_region does; with levels < 5 the field's grid is coarser than the working
 * size, which the same rule covers. From there on the frame is §6.13's: its bytes and kept state are those of the same sequence with nct_seq_set_region(M_t) called
 * before it. The field is zero — the matte stays, the age still counts — with motion off, in a sequence without state (a first frame, after nct_seq_reset) and on a
 * CUT frame of nct_seq_frame_auto: AFTER A CUT THE CALLER SHOULD SET A NEW MATTE, the old one marks a place in a shot that is over. A full frame finds its fields ahead
 * of its level masks whether or not it blends (tau == 0 too); the carry's time counts in other_ms. A coarse field holds whole vectors of its own grid: a pan of a
 * fraction of a cell per frame does not move the matte (SPEC §6.14 rule 5). Turning tracking off leaves the matte in force as a sticky §6.13 matte. The first carry
 * reserves one second matte block at the size frames arrive; the two change places. Never turned on, or no matte set: every sequence path is what it was.
 * nct_seq_get_region: the matte in force at the size frames arrive (a full-resolution sequence: the original size) and, through `age` (nullable), the frames run since
 * the matte's own frame while tracking was on. No open sequence or no matte: NCT_ERR_STATE. Synchronous.
 * Not defined: occlusion handling or a confidence for the carried matte, sub-pixel motion, and which of the two mattes stays after a frame that fails (such a frame
 * leaves the sequence reset). */
int nct_seq_matte_warp(nct_ctx* ctx, const uint8_t* mask_prev /* H*W */, int H, int W, const int16_t* field /* h*w*2 */, int h, int w, uint8_t* mask_out /* H*W */);
int nct_seq_matte_warp_dev(nct_ctx* ctx, const uint8_t* d_mask_prev, int H, int W, const int16_t* d_field, int h, int w, uint8_t* d_mask_out);
int nct_seq_set_region_tracking(nct_ctx* ctx, int on);
int nct_seq_get_region(nct_ctx* ctx, uint8_t* mask_out, int* age);

/* ---- matte snapping (SPEC §6.15; an extension): a carried matte is re-fitted to the colours of the frame it now belongs to — a joint filter over the matte with the
 * frame's 8-bit Lab image as the guide, in integers only.
 * nct_region_snap[_dev]: mask: H x W bytes; lab: the 8-bit Lab image (nct_bgr2lab_u8) of the same frame at the same size, H x W x 3; 1 <= H, W <= 16384, H * W <= 2^26
 * (nct_seq_matte_warp's target limits); params NULL: the defaults (radius 3, sigma 10, binary 1); radius in [1, 8], sigma in [1, 255] (8-bit Lab units), binary in {0, 1}.
 * Per pixel p and tap q = p + (dy, dx), dy, dx = -radius … radius, taps outside the image skipped: d2 = the squared distance of lab(p) and lab(q) over the three bytes,
 * w(q) = max(0, 3 sigma^2 - d2), A = sum w(q) mask(q), B = sum w(q) (the centre tap weighs 3 sigma^2: B > 0); v = floor((2A + B) / (2B)), the mean rounded half up;
 * mask_out(p) = v, or with binary set v >= 128 ? 255 : 0. A constant matte comes back as it is; with binary 0 every byte lies between the least and the largest
 * byte of its window; a guide whose every pixel is at least 3 sigma^2 away from all its neighbours returns the matte; a flat guide makes the pass a box mean (binary: a
 * majority filter). The host form is synchronous; the _dev form is enqueued on the context's stream and refuses a mask_out that overlaps mask or lab (the pass
 * gathers). A null pointer, a side or a parameter out of range are NCT_ERR_INVALID, the message names the argument.
 * nct_seq_set_region_snap: on an open sequence, between frames; non-NULL turns snapping on with these parameters, NULL turns it off (the default). Bad parameters are
 * NCT_ERR_INVALID and leave the setting as it was; no open sequence is NCT_ERR_STATE. Snapping acts only while tracking is on and a matte is set: on every frame on
 * which the matte's age counts (not the matte's own frame) in a sequence with state — not on a first frame, a frame after nct_seq_reset or a CUT frame — the matte is
 * snapped behind the carry, M_t = snap(matte_warp(M_(t-1), field), Lab(S_t)), with motion on or off (off: the field is zero, the snap alone re-fits the matte). The
 * guide is nct_bgr2lab_u8 of the frame at the size frames arrive: a full-resolution sequence snaps at the original size, before the shrink to the working-size matte.
 * From there on the frame is §6.13's, its bytes and kept state those of the same sequence with nct_seq_set_region(M_t) called before it; nct_seq_get_region returns
 * the snapped matte; the snap's time counts in other_ms. It reserves nothing for the life of the sequence beside tracking's second matte block. A MATTE DRAWN ON NOTHING
 * HAS NOTHING TO SNAP TO: a region that is texture, not an object of its own colour, erodes. Never turned on: every sequence path is what it was. */
typedef struct nct_region_snap_params { int radius, sigma, binary; } nct_region_snap_params;
void nct_region_snap_params_default(nct_region_snap_params* p);     /* radius 3, sigma 10, binary 1 */
int nct_region_snap(nct_ctx* ctx, const uint8_t* mask /* H*W */, const uint8_t* lab /* H*W*3 */, int H, int W, const nct_region_snap_params* params, uint8_t* mask_out /* H*W */);
int nct_region_snap_dev(nct_ctx* ctx, const uint8_t* d_mask, const uint8_t* d_lab, int H, int W, const nct_region_snap_params* params, uint8_t* d_mask_out);
int nct_seq_set_region_snap(nct_ctx* ctx, const nct_region_snap_params* params);

/* ---- region selection from strokes (SPEC §6.16; an extension): the matte the region calls above take, made from a few marked pixels and the VGG19 features the
 * correspondence is built on. strokes has one byte per source pixel: NCT_STROKE_IN marks "inside the object", NCT_STROKE_OUT "outside", every other value is unmarked.
 * nct_region_select[_dev]: src_bgr h x w x 3 (sides in nct_pair_upload's range [17, 4000]), strokes and mask_out h x w. params NULL: the defaults (tap 2, sharpness 1024,
 * floor_permille 700, max_seeds 4096, snap_iters 1, snap = nct_region_snap_params_default); tap in [1, 5], sharpness in [1, 65536], floor_permille in [0, 1000], max_seeds
 * in [1, 4096], snap_iters in [0, 8], snap as nct_region_snap takes it.
 * (1) F = tap `tap` of nct_vgg19_features(src) on its grid h_t x w_t, h_t = ((h - 1) >> (tap - 1)) + 1, with C channels; u = nct_feat_normalize(F).
 * (2) q(p)[c] = (int16) rint(u(p)[c] * 32767), the product in fp32; a non-finite u (the zero-norm pixel) gives 0. |q| < 32780, so every dot product of two rows and every
 *     partial sum of it stays below 2^31: int32 sums are exact in any order.
 * (3) Source pixel (y, x) belongs to cell (y >> (tap - 1), x >> (tap - 1)). A cell with an IN pixel and no OUT pixel is an inside seed, the reverse an outside seed, one
 *     with both is mixed and no seed. A class with n > max_seeds seeds keeps the seed of raster rank i iff floor((i + 1) max_seeds / n) > floor(i max_seeds / n): exactly max_seeds.
 * (4) Per cell p: s_in = the largest dot product q(p) . q(s) over the kept inside seeds s, s_out the same over the kept outside seeds, or floor(floor_permille 2^30 / 1000)
 *     without any; d = s_in - s_out; m(p) = clamp(128 + floor((d sharpness + 2^29) / 2^30), 0, 255) in 64 bits. Then every inside seed cell, kept or not, is 255 and every
 *     outside seed cell 0.
 * (5) M = nct_resize_u8c1(m -> h x w); at tap 1 a copy.
 * (6) The stamp sets IN pixels to 255 and OUT pixels to 0; then snap_iters times M = nct_region_snap(M, nct_bgr2lab_u8(src), snap) and the stamp again.
 * Integers from (2) on: the result does not depend on any summation order. nct_region_select: host pointers, synchronous; stages (nullable, its arrays nullable) receives
 * q [cells][C], per cell the code 0 none, 1 inside kept, 2 outside kept, 3 inside not kept, 4 outside not kept, 5 mixed, m on the tap grid and M after (5).
 * nct_region_select_dev: device pointers, no stages; it waits once, for the two seed counts (the refusal and the launch shapes need them), and returns with the rest
 * enqueued. All transients come from the arena and go back in stream order; nothing is kept. NCT_ERR_STATE: no weights loaded. NCT_ERR_INVALID with a message naming the
 * argument: a null pointer, a side or a parameter out of range; and "no inside seed cell" where no cell is an inside seed (an IN stroke that lies only in mixed cells too).
 * nct_feat_quantize: (2) alone behind N1, CHW fp32 in like nct_feat_normalize, [H*W][C] int16 out; nct_feat_quantize_dev: HWC in. C a positive multiple of 4.
 * nct_region_score[_dev]: (4) without the seed-cell overwrite. q [cells][C], seeds_in [n_in][C], seeds_out [n_out][C] (nullable with n_out = 0) int16, rows with |row| < 32780
 * (not checked: a longer row may wrap an int32 sum); cells in [1, 2^24], C a multiple of 4 in [4, 4096], n_in in [1, 65536], n_out in [0, 65536]; score_out [cells] bytes.
 * The _dev form reads rows in 8-byte units: its three arrays must be 8-byte aligned (arena blocks are).
 * nct_pair_select_region: after nct_pair_upload / nct_multi_upload, nct_region_select on the uploaded source followed by nct_pair_set_region(matte, region), the matte never
 * leaving the device; its refusals are those two calls'. nct_seq_select_region: on a sequence opened with nct_seq_begin, nct_region_select on frame_bgr (a frame of the
 * sequence's size; it is not run) followed by nct_seq_set_region: the matte belongs to the next frame that runs, and tracks and snaps from there. In a full-resolution
 * sequence: NCT_ERR_STATE with a message (selection at an original size above 4000 is not defined).
 * THE RULE WAS TRIED WITH SYNTHETIC WEIGHTS ONLY; nobody has measured it with the Oxford weights. */
#define NCT_STROKE_IN 255
#define NCT_STROKE_OUT 128
typedef struct nct_region_select_params { int tap, sharpness, floor_permille, max_seeds, snap_iters; nct_region_snap_params snap; } nct_region_select_params;
void nct_region_select_params_default(nct_region_select_params* p);     /* 2, 1024, 700, 4096, 1, {3, 10, 1} */
typedef struct nct_region_select_stages { int16_t* q; uint8_t* cell; uint8_t* score; uint8_t* up; } nct_region_select_stages;   /* [cells][C]; [cells]; [cells]; [h*w]; all nullable */
int nct_region_select(nct_ctx* ctx, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params, uint8_t* mask_out,
                      const nct_region_select_stages* stages);
int nct_region_select_dev(nct_ctx* ctx, const uint8_t* d_src_bgr, int h, int w, const uint8_t* d_strokes, const nct_region_select_params* params, uint8_t* d_mask_out);
int nct_feat_quantize(nct_ctx* ctx, const float* src_chw, int16_t* dst, int C, int H, int W);
int nct_feat_quantize_dev(nct_ctx* ctx, const float* d_src_hwc, int16_t* d_dst, int C, int H, int W);
int nct_region_score(nct_ctx* ctx, const int16_t* q, int cells, int C, const int16_t* seeds_in, int n_in, const int16_t* seeds_out, int n_out, int sharpness, int floor_permille,
                     uint8_t* score_out);
int nct_region_score_dev(nct_ctx* ctx, const int16_t* d_q, int cells, int C, const int16_t* d_seeds_in, int n_in, const int16_t* d_seeds_out, int n_out, int sharpness,
                         int floor_permille, uint8_t* d_score_out);
int nct_pair_select_region(nct_ctx* ctx, const uint8_t* strokes, const nct_region_select_params* params, const nct_region_params* region);
int nct_seq_select_region(nct_ctx* ctx, const uint8_t* frame_bgr, const uint8_t* strokes, const nct_region_select_params* params, const nct_region_params* region);

/* ---- region models (SPEC §6.17; an extension): what a selection from strokes learnt — the kept seed rows of §6.16 rule 3 — held so that the object is found again on
 * another image, or on every full frame of a shot, without new strokes. nct_region_model is a host object without a context, like nct_model: the tap, C, the kept inside
 * rows [n_in][C] and the kept outside rows [n_out][C] as int16, in the raster order of §6.16 rule 3, image after image.
 * nct_region_model_fit: §6.16 rules (1) to (3) on src_bgr and strokes; the kept rows become a new model. Of the params only tap and max_seeds act; the limits and
 * refusals are nct_region_select's, "no inside seed cell" included. nct_region_model_add: the same on another image, its kept rows appended behind the model's; a tap
 * other than the model's, or a class that would exceed 65536 rows (nct_region_score's limit), is NCT_ERR_INVALID; a refused call leaves the model unchanged.
 * nct_region_model_info: tap, C, n_in, n_out (each nullable). nct_region_model_rows: host pointers to the rows (rows_out NULL without outside rows), valid until the next
 * nct_region_model_add or nct_region_model_free. nct_region_model_from_rows: a model from rows the caller holds (a saved model, rows made by another program); needs no
 * context; tap in [1, 5], C the tap's channel count (64, 128, 256, 512, 512), n_in in [1, 65536], n_out in [0, 65536]; rows are copied. The three calls without a
 * context report a refusal through nct_last_error(NULL).
 * nct_region_refind[_dev]: the re-find step alone. score: ht x wt bytes on the tap grid; prior: H x W bytes or NULL; out: H x W bytes.
 * (R1) r = nct_resize_u8c1(score: ht x wt -> H x W); equal sizes give the byte itself; the target is never smaller than the grid.
 * (R2) confident(p) = r(p) >= 128 + margin or r(p) < 128 - margin, in integers, margin in [0, 128].
 * (R3) out(p) = (prior == NULL or confident(p)) ? r(p) : prior(p).
 * margin 0 or a NULL prior give nct_resize_u8c1's bytes, margin 128 the prior; a byte is r's or the prior's, never a mix. 1 <= ht <= H <= 16384, 1 <= wt <= W <= 16384,
 * ht, wt <= 4096, H * W <= 2^26; anything else is NCT_ERR_INVALID, the message names the argument. One kernel, no intermediate of the target's size. The _dev form is
 * enqueued on the context's stream and refuses an out that overlaps score or prior.
 * nct_region_model_apply[_dev]: src_bgr h x w x 3 (sides in [17, 4000]), prior h x w or NULL, mask_out h x w. params NULL: the defaults (sharpness 1024, floor_permille
 * 700, margin 32, snap_iters 1, snap = nct_region_snap_params_default); the ranges are §6.16's and (R2)'s.
 * (A1) q = §6.16 rules (1) and (2) on the image at the model's tap. (A2) m = nct_region_score(q, rows_in, rows_out, sharpness, floor_permille): no cell of this image is
 * a seed cell, nothing is overwritten. (A3) M = refind(m, prior, margin) at h x w. (A4) snap_iters times M = nct_region_snap(M, nct_bgr2lab_u8(src), snap); no stamp.
 * stages (nullable, its arrays nullable; host form only) receives q [cells][C], m on the tap grid and M after (A3). NCT_ERR_STATE: no weights loaded. The _dev form
 * waits once, for the model's rows to be on the device (the model may be changed or freed on return), and returns with the rest enqueued; it refuses a mask_out that
 * overlaps src_bgr or prior. All transients come from the arena and go back in stream order; nothing is kept.
 * nct_pair_apply_region_model: after nct_pair_upload / nct_multi_upload, nct_region_model_apply without a prior on the uploaded source followed by
 * nct_pair_set_region(matte, region), the matte never leaving the device; its refusals are those two calls'.
 * nct_seq_set_region_model: on an open sequence, between frames, a full-resolution sequence included; the model's rows are copied to the device once and held until
 * the model is replaced, removed (model NULL), nct_seq_end or nct_destroy — the model itself may be freed on return. params and region as above (region: the protect of
 * the re-found matte); bad parameters are NCT_ERR_INVALID and leave the setting as it was; no open sequence is NCT_ERR_STATE. While a model is set:
 * (S1) a frame that is a fresh matte's own frame (§6.14) uses that matte as it came: no re-find. (S2) Every other full frame — nct_seq_frame* and the FIRST, KEY and CUT
 *      frames of nct_seq_frame_auto — re-finds at the working size: q comes from the model's tap of the frame's own forward, which also stores that tap channel-last;
 *      there is no second forward. (S3) The prior is the matte that §6.14 and §6.15 leave for this frame, at the size frames arrive; none where the sequence has no state
 *      (a first frame, a frame after nct_seq_reset, a CUT frame: the old shot's matte is not evidence) or no matte is set. (S4) M_t = refind(m, prior, margin) straight
 *      from the working-size tap grid to the size frames arrive — the original size in a full-resolution sequence —, then (A4)'s snap passes with the frame's Lab image
 *      at that size; a full-resolution sequence then shrinks M_t with nct_resize_u8c1, as nct_seq_set_region does. (S5) From there the frame is §6.13's: its bytes and
 *      kept state are those of the same sequence with nct_seq_set_region(M_t, region) called before it; nct_seq_get_region returns M_t; a matte the re-find made where
 *      none was set has age 0 on that frame, else the age counts as in §6.14; the re-find's time counts in other_ms. (S6) Propagated frames run no forward and do not
 *      re-find: they carry and snap as before. nct_seq_probe's record and the decisions of nct_seq_frame_auto do not depend on the model. A frame that fails leaves the
 *      sequence reset and the model set. Never set: every sequence path is what it was.
 * WHERE THE SCORE ALONE FAILS (an object whose appearance changed) A CARRIED MATTE AS THE PRIOR IS THE REMEDY, AND A LAGGING PRIOR COSTS ACCURACY AS THE MARGIN GROWS;
 * margin 32 balanced the two on one synthetic fixture WITH SYNTHETIC WEIGHTS. Nobody has measured the rule with the Oxford weights. */
typedef struct nct_region_model nct_region_model;
typedef struct nct_region_refind_params { int sharpness, floor_permille, margin, snap_iters; nct_region_snap_params snap; } nct_region_refind_params;
void nct_region_refind_params_default(nct_region_refind_params* p);     /* 1024, 700, 32, 1, {3, 10, 1} */
typedef struct nct_region_apply_stages { int16_t* q; uint8_t* score; uint8_t* refound; } nct_region_apply_stages;   /* [cells][C]; [cells]; [h*w]; all nullable */
int nct_region_model_fit(nct_ctx* ctx, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params, nct_region_model** model);
int nct_region_model_add(nct_ctx* ctx, nct_region_model* model, const uint8_t* src_bgr, int h, int w, const uint8_t* strokes, const nct_region_select_params* params);
int nct_region_model_info(const nct_region_model* model, int* tap, int* C, int* n_in, int* n_out);
int nct_region_model_rows(const nct_region_model* model, const int16_t** rows_in, const int16_t** rows_out);
int nct_region_model_from_rows(int tap, int C, const int16_t* rows_in, int n_in, const int16_t* rows_out, int n_out, nct_region_model** model);
void nct_region_model_free(nct_region_model* model);
int nct_region_refind(nct_ctx* ctx, const uint8_t* score, int ht, int wt, const uint8_t* prior /* H*W, nullable */, int H, int W, int margin, uint8_t* out /* H*W */);
int nct_region_refind_dev(nct_ctx* ctx, const uint8_t* d_score, int ht, int wt, const uint8_t* d_prior, int H, int W, int margin, uint8_t* d_out);
int nct_region_model_apply(nct_ctx* ctx, const nct_region_model* model, const uint8_t* src_bgr, int h, int w, const uint8_t* prior /* h*w, nullable */,
                           const nct_region_refind_params* params, uint8_t* mask_out, const nct_region_apply_stages* stages);
int nct_region_model_apply_dev(nct_ctx* ctx, const nct_region_model* model, const uint8_t* d_src_bgr, int h, int w, const uint8_t* d_prior, const nct_region_refind_params* params,
                               uint8_t* d_mask_out);
int nct_pair_apply_region_model(nct_ctx* ctx, const nct_region_model* model, const nct_region_refind_params* params, const nct_region_params* region);
int nct_seq_set_region_model(nct_ctx* ctx, const nct_region_model* model, const nct_region_refind_params* params, const nct_region_params* region);

/* ---- reference libraries (SPEC §6.21; an extension): which of many graded stills suit a source. Every multi-reference call above begins with the caller naming the
 * references; a reference with nothing in it that matches the source is the usual way the method fails. A library holds, per still, the int8 descriptors of one VGG19
 * tap; ranking a source against it is one dense integer GEMM with a max epilogue per entry, on the int8 matrix cores, exact in every bit.
 * (D1) F = tap `tap` (1 … 5) of nct_vgg19_features(image), C channels, on the grid h_t x w_t of §6.16 rule 1; cells = h_t w_t must lie in [1, 65536].
 * (D2) g(p) = F(p) - mu in fp32 (mu: the library's centre, fp32 [C], or none), u = N1(g) with nct_feat_normalize's summation, d(p)[c] = (int8) rint(u(p)[c] * 127), the
 *      product in fp32; a non-finite u gives 0.
 * (D3) P = A B^T in int32 for the source's rows A [na][C] and an entry's rows B [nb][C]; fwd = sum_p max_q P[p][q], bwd = sum_q max_p P[p][q], both int64.
 * (D4) key = wf floor(fwd 1024 / na) + wb floor(bwd 1024 / nb) in int64, wf and wb integers in [0, 16], not both 0 (default 1, 1: coherence and completeness, as in the
 *      BDS vote); the order is by descending key, the lower index first on a tie.
 * nct_feat_quantize8[_dev]: (D2) alone. src_chw: a Caffe blob [C][H][W] (the _dev form: channel-last [H*W][C]); center: [C] or NULL; dst: [H*W][C] int8. C a multiple
 * of 16 in [16, 4096], H, W in [1, 4096].
 * nct_descriptor_match[_dev]: (D3) alone. a: [na][C]; rows: the entries' rows end to end, entry k the rows offsets[k] … offsets[k + 1] - 1 (offsets: int32 [N + 1],
 * offsets[0] = 0); fwd, bwd: int64 [N]. 1 <= na <= 65536, every entry 1 … 65536 rows, N in [1, 4096], C as above, all rows at most 2^31 bytes. In the _dev form a and
 * rows are device pointers aligned to 16 bytes, fwd and bwd device pointers aligned to 8, and offsets stays a HOST array: the limits are checked on it, then it goes
 * up and is waited for, the launches are enqueued on the context's stream.
 * nct_reflib is a host object without a context, like nct_region_model: tap, C, the centre (copied) and the entries' rows with their offsets.
 * nct_reflib_create: an empty library; C must be the tap's channel count. nct_reflib_add: (D1) and (D2) on bgr (h x w x 3, sides in nct_pair_upload's range [17, 4000]) —
 * one forward to the tap —, the rows appended as a new entry; NCT_ERR_STATE without weights. nct_reflib_info: tap, C, N, the total rows, whether centred (each
 * nullable). nct_reflib_rows: host pointers to the rows, the offsets and the centre (NULL without), valid until the next nct_reflib_add or nct_reflib_free.
 * nct_reflib_from_rows: a library from rows the caller holds (a saved library); needs no context; everything is copied. The calls without a context report a refusal
 * through nct_last_error(NULL).
 * nct_reflib_rank: one forward of src_bgr (sides in [17, 4000]) to the library's tap, (D2) with the library's centre, (D3) against every entry, (D4). order: int32 [N];
 * key, fwd, bwd: int64 [N], each nullable. params NULL: wf 1, wb 1. The context keeps the library's rows on the device in arena blocks, keyed by the library and a
 * revision counter every add bumps: a second rank against an unchanged library uploads nothing. nct_reflib_release, a rank against another library and nct_destroy give
 * the blocks back. It works with a pair uploaded or a sequence open and touches neither. Synchronous.
 * Every refusal is NCT_ERR_INVALID (NCT_ERR_STATE: no weights) with a message that names the argument, before anything is reserved or enqueued.
 * THE RULE RANKED FIVE ONE-TEXTURE STILLS CORRECTLY WITH SYNTHETIC WEIGHTS, AND CENTRING ON THE LIBRARY'S MEAN TAP VECTOR WIDENED THE MARGINS. Nobody has
 * measured the rule with the Oxford weights or on photographs. */
typedef struct nct_reflib nct_reflib;
typedef struct nct_reflib_params { int wf, wb; } nct_reflib_params;
void nct_reflib_params_default(nct_reflib_params* p);                   /* 1, 1 */
int nct_feat_quantize8(nct_ctx* ctx, const float* src_chw, const float* center /* [C], nullable */, int8_t* dst, int C, int H, int W);
int nct_feat_quantize8_dev(nct_ctx* ctx, const float* d_src_hwc, const float* d_center, int8_t* d_dst, int C, int H, int W);
int nct_descriptor_match(nct_ctx* ctx, const int8_t* a, int na, int C, const int8_t* rows, const int32_t* offsets /* [N + 1] */, int N, int64_t* fwd, int64_t* bwd);
int nct_descriptor_match_dev(nct_ctx* ctx, const int8_t* d_a, int na, int C, const int8_t* d_rows, const int32_t* offsets /* HOST, [N + 1] */, int N, int64_t* d_fwd, int64_t* d_bwd);
int nct_reflib_create(int tap, int C, const float* center /* [C], nullable */, nct_reflib** lib);
int nct_reflib_add(nct_ctx* ctx, nct_reflib* lib, const uint8_t* bgr, int h, int w);
int nct_reflib_info(const nct_reflib* lib, int* tap, int* C, int* N, int64_t* total_rows, int* centred);
int nct_reflib_rows(const nct_reflib* lib, const int8_t** rows, const int32_t** offsets, const float** center);
int nct_reflib_from_rows(int tap, int C, const float* center /* [C], nullable */, const int8_t* rows, const int32_t* offsets /* [N + 1] */, int N, nct_reflib** lib);
void nct_reflib_free(nct_reflib* lib);
int nct_reflib_rank(nct_ctx* ctx, const nct_reflib* lib, const uint8_t* src_bgr, int h, int w, const nct_reflib_params* params, int32_t* order, int64_t* key, int64_t* fwd,
                    int64_t* bwd);
int nct_reflib_release(nct_ctx* ctx);

/* ---- device-pointer seams: the same operations on buffers that stay in HBM between calls (main.cu:204-316 keeps Ndata_C1, ann_device, ... on the device
 * across these kernels; an integrator replacing single seams should not pay H2D + D2H + a synchronise per call). Buffers come from the context's arena
 * (nct_dev_alloc / nct_dev_free; any device pointer of the context's GPU works as an operand). Calls are enqueued on the context's stream in call order and return
 * immediately; nct_dev_download and nct_synchronize wait. Arena blocks are recycled in the order of THAT stream: use them from another stream (or free them while your own
 * kernels still read them) only after nct_synchronize. nct_dev_free of a pointer that is not a live nct_dev_alloc block of the context returns NCT_ERR_INVALID. Features: channel-last HWC fp32 (nct_chw_to_hwc_dev converts a Caffe blob once); `unit_norm` = 1
 * tells nct_patchmatch_bidir_dev that both maps hold unit vectors (output of nct_feat_normalize_dev), which enables the exact row-wise rejection.
 * Chained like the reference's level loop they reproduce nct_pair_run_levels bit for bit (tests/test_gpu_pipeline.py::test_dev_seams_chain_equals_pipeline).
 * Limits, each refused with NCT_ERR_INVALID and a message naming the entry point before anything is reserved or enqueued (tests/test_gpu_dev_seams.py::test_refusals):
 *  - every non-nullable pointer is set (nullable: resp, pw, dims, d_taps_chw, d_taps_hwc and their entries); nnf_half != nnf;
 *  - maps [C][H][W] / [H][W][C]: C, H, W >= 1 with H * W and C * H * W at most 2^31 - 256; C a multiple of 4 for normalise, matching error, PatchMatch and the feature
 *    vote, C <= 512 for the feature vote;
 *  - fields (NNF init / upsample, PatchMatch, both votes): 1 <= ah, aw, bh, bw (and ah_half, aw_half) < 4096, the NNF word holds 12 bits per coordinate; ah, aw >= 2 for
 *    nct_nnf_init_dev; patch = 3; iters, rs_max >= 0;
 *  - images: 2 <= h, w < 4096, stride (bytes from one row to the next; rows need no alignment) >= 3 w, deepest_tap in 1..5.
 * nct_bds_vote_features and nct_bds_vote_image, the host forms of the votes, take the same field dimensions. */
int nct_dev_alloc(nct_ctx* ctx, size_t bytes, void** out);
int nct_dev_free(nct_ctx* ctx, void* p);
int nct_dev_upload(nct_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int nct_dev_download(nct_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int nct_chw_to_hwc_dev(nct_ctx* ctx, const float* src_chw, float* dst_hwc, int C, int H, int W);
int nct_hwc_to_chw_dev(nct_ctx* ctx, const float* src_hwc, float* dst_chw, int C, int H, int W);
int nct_vgg19_features_dev(nct_ctx* ctx, const uint8_t* d_bgr, int h, int w, int stride, int deepest_tap, float* const* d_taps_chw, int* dims);   /* main.cu:94,102,426 */
/* the same forward with the taps ALSO / INSTEAD channel-last (d_taps_hwc[t], nullable like d_taps_chw[t], which may itself be NULL): the tap layer's own epilogue writes the HWC map
 * the correspondence seams below read, so an integrator who does not need Caffe's planar blobs skips nct_chw_to_hwc_dev altogether */
int nct_vgg19_features_hwc_dev(nct_ctx* ctx, const uint8_t* d_bgr, int h, int w, int stride, int deepest_tap, float* const* d_taps_chw, float* const* d_taps_hwc, int* dims);
int nct_feat_normalize_dev(nct_ctx* ctx, const float* src_hwc, float* dst_hwc, float* resp, int C, int H, int W);                                    /* main.cu:265,274,313 */
int nct_nnf_init_dev(nct_ctx* ctx, uint32_t* nnf, int ah, int aw, int bh, int bw);                                                                    /* main.cu:232-233 */
int nct_nnf_upsample_dev(nct_ctx* ctx, const uint32_t* nnf_half, uint32_t* nnf, int ah, int aw, int bh, int bw, int ah_half, int aw_half);           /* main.cu:240-250 */
int nct_patchmatch_dev(nct_ctx* ctx, const float* a_hwc, const float* b_hwc, int C, int ah, int aw, int bh, int bw, int patch, int iters, int rs_max,
                       uint32_t seed, uint32_t* nnf, float* dist);                                                                                     /* main.cu:283 */
int nct_patchmatch_bidir_dev(nct_ctx* ctx, const float* a_hwc, const float* b_hwc, int C, int ah, int aw, int bh, int bw, int patch, int iters, int rs_max,
                             uint32_t seed_ab, uint32_t seed_ba, uint32_t* ann, float* annd, uint32_t* bnn, float* bnnd, int unit_norm);              /* main.cu:283-284 */
int nct_bds_vote_features_dev(nct_ctx* ctx, const uint32_t* ann, const uint32_t* bnn, const float* pin_hwc, float* pout_hwc, float* pw, int C, int ah, int aw,
                              int bh, int bw, int patch, float w_coherence, float w_complete);                                                         /* main.cu:303-311 */
int nct_bds_vote_image_dev(nct_ctx* ctx, const uint8_t* b_bgr, const uint32_t* ann, const uint32_t* bnn, int ah, int aw, int bh, int bw, int patch,
                           double w_coherence, double w_complete, uint8_t* out_bgr);                                                                   /* main.cu:291 */
int nct_feature_distance_dev(nct_ctx* ctx, const float* a_hwc, const float* b_hwc, float* err, int C, int H, int W);                                  /* main.cu:316 */
/* One 3x3 / pad 1 / stride 1 conv layer (+ bias, ReLU if `relu`) through the launcher the VGG forward uses, with every store form of its kernel: d_out_chw planar [Cout][H][W],
 * d_out_hwc channel-last [H*W][Cout], either or both (one may be null); pool = 1: d_out_chw receives only the 2x2/2 ceil-mode max-pooled map [Cout][(H-1)/2+1][(W-1)/2+1]
 * and d_out_hwc must be null. d_weights: Caffe layout [Cout][Cin][3][3] on the device (packed by the call into an arena block of its own), d_bias [Cout]. Cout % 64 == 0,
 * 1 <= H, W < 4096. The kernel consumes input channels in pairs: for an odd Cin, d_in must hold Cin + 1 planes and the CALLER zeroes the last one (the call neither copies nor writes
 * the input). nct_conv3x3_pair_dev: the same layer for two maps of different size; one launch where both grids are too small to fill the GPU (and NCT_CONV_PAIR is not 0),
 * two launches otherwise; the bits are the same either way. Per map one of the two outputs may be null. No pooling. */
int nct_conv3x3_dev(nct_ctx* ctx, const float* d_in, const float* d_weights, const float* d_bias, int Cin, int Cout, int H, int W, int relu, int pool,
                    float* d_out_chw, float* d_out_hwc);
int nct_conv3x3_pair_dev(nct_ctx* ctx, const float* d_in1, int H1, int W1, const float* d_in2, int H2, int W2, const float* d_weights, const float* d_bias, int Cin, int Cout,
                         int relu, float* d_out1, float* d_out2, float* d_hwc1, float* d_hwc2);

/* ---- correspondence carry in frame sequences (SPEC §6.23) ----
 * A full frame of a sequence starts every level's PatchMatch from nct_nnf_init or the upsampled coarser field. With the carry on, the sequence also keeps the final
 * fields of every level run (per reference) of its last full frame, moves them along the level's backward motion field on every frame (with motion off they stay where
 * they are), and a full frame merges them into the level's start field: per query the kept match replaces the ordinary start where its step-0 patch distance is
 * strictly smaller (fp32; a NaN keeps the ordinary start). The level's PatchMatch then runs unchanged on that start field, with `iters` iterations on a frame that
 * merged. The first frame, and the first after nct_seq_reset or a cut of nct_seq_frame_auto, has nothing to merge and is the frame the sequence gives without the carry.
 * nct_seq_set_carry: on in {0, 1}; iters in [0, 64], or -1 for the sequence's pm_iters. Turning the carry on reserves the kept fields, the forward map and one scratch
 * field; turning it off gives them back. No open sequence: NCT_ERR_STATE; a value out of range: NCT_ERR_INVALID; a refused call changes nothing. A sequence that never
 * calls it keeps its bytes, launches and arena exactly. NCT_VERSION stays 118: entry points were only added.
 * nct_seq_get_carry: the kept fields of reference k at level run l — ann [ah_l*aw_l] on the source's level grid, bnn [bh_l*bw_l] on the reference's, either pointer
 * nullable — as the last frame left them; NCT_ERR_STATE where the sequence holds none (carry off, before the first full frame, after a reset or cut).
 * The seams, on host arrays (synchronous) and as _dev forms on device pointers (enqueued). Fields are int16 [h*w][2] of (my, mx); NNF words are (y << 12) | x:
 *   nct_nnf_carry        nnf_out(p) = nnf_prev(p + m(p)), the vector clamped component-wise so that p + m is inside.
 *   nct_nnf_forward_map  fwd_out(s) = min { word(p) : p + m(p) = s } with the same clamp, and word(clamp(s - m(s))) where no p lands on s.
 *   nct_nnf_remap        bnn_out(q) = fwd(bnn_prev(q)) on the grid bh x bw, fwd on h x w; a word whose coordinates leave h x w is clamped to it.
 *   nct_nnf_merge        one direction of the merge: a / b normalised features (host form: [C][ah][aw] and [C][bh][bw] as nct_patchmatch takes them; _dev: channel-last),
 *                        z the ordinary start field and c the moved kept field, both [ah*aw] words into b's grid; start_out [ah*aw]; dz_out / dc_out (nullable) the two
 *                        step-0 distances, bit for bit what nct_patchmatch(iters = 0) returns for z and c. patch must be 3.
 * The _dev forms gather on the caller's blocks and refuse (NCT_ERR_INVALID) an output block that overlaps an input block: nnf_out and nnf_prev, fwd_out and field,
 * bnn_out and bnn_prev or fwd, start_out and z or c. The host forms stage every array in device blocks of their own and never look at how the host arrays lie. */
int nct_seq_set_carry(nct_ctx* ctx, int on, int iters);
int nct_seq_get_carry(nct_ctx* ctx, int k, int l, uint32_t* ann, uint32_t* bnn);
int nct_nnf_carry(nct_ctx* ctx, const uint32_t* nnf_prev, int h, int w, const int16_t* field, uint32_t* nnf_out);
int nct_nnf_carry_dev(nct_ctx* ctx, const uint32_t* d_nnf_prev, int h, int w, const int16_t* d_field, uint32_t* d_nnf_out);
int nct_nnf_forward_map(nct_ctx* ctx, const int16_t* field, int h, int w, uint32_t* fwd_out);
int nct_nnf_forward_map_dev(nct_ctx* ctx, const int16_t* d_field, int h, int w, uint32_t* d_fwd_out);
int nct_nnf_remap(nct_ctx* ctx, const uint32_t* bnn_prev, int bh, int bw, const uint32_t* fwd, int h, int w, uint32_t* bnn_out);
int nct_nnf_remap_dev(nct_ctx* ctx, const uint32_t* d_bnn_prev, int bh, int bw, const uint32_t* d_fwd, int h, int w, uint32_t* d_bnn_out);
int nct_nnf_merge(nct_ctx* ctx, const float* a_chw, const float* b_chw, int C, int ah, int aw, int bh, int bw, int patch, const uint32_t* z, const uint32_t* c,
                  uint32_t* start_out, float* dz_out, float* dc_out);
int nct_nnf_merge_dev(nct_ctx* ctx, const float* d_a_hwc, const float* d_b_hwc, int C, int ah, int aw, int bh, int bw, int patch, const uint32_t* d_z, const uint32_t* d_c,
                      uint32_t* d_start_out, float* d_dz_out, float* d_dc_out);

/* ---- measurement hooks (bench.py / rocprof): device-resident PatchMatch on synthetic features ----
 * nct_pm_bench_setup uploads + normalises two CHW feature maps once; nct_pm_bench_run re-initialises the NNF
 * (scaled identity) and runs one full nct_patchmatch pass (init-dist + iters*4 Jacobi steps) entirely on the
 * device, returning the kernel time of that pass measured with HIP events on the library's own stream and the
 * number of distance evaluations actually performed (device counter). */
int nct_pm_bench_setup(nct_ctx* ctx, const float* a_chw, const float* b_chw, int C, int ah, int aw, int bh, int bw);
int nct_pm_bench_run(nct_ctx* ctx, int iters, int rs_max, uint32_t seed, float* kernel_ms, uint64_t* evals, uint32_t* nnf_out, float* dist_out);
/* the pipeline's form of the same pass: both directions fused per launch; pm_mode 0 = fp32 tiles, 1 = fp32 tiles + exact row-wise
 * rejection for unit-norm features (the pipeline's default), 2 = fp16 tiles (NCT_FLAG_FEAT16). counters (nullable, 2 x uint64):
 * evaluations, accepted candidates. */
int nct_pm_bench_run_bidir(nct_ctx* ctx, int iters, int rs_max, uint32_t seed, int pm_mode, float* kernel_ms, uint64_t* counters, uint32_t* ann_out, float* annd_out,
                           uint32_t* bnn_out, float* bnnd_out);
/* the score kernel of region selection alone (SPEC §6.16 rule 4; scripts/region_select_times.py): nct_region_score_dev's arguments; one warm-up launch, then `reps`
 * launches (1 … 1000) between two HIP events on the library's own stream; kernel_ms receives the mean device time of one launch. Synchronous. */
int nct_region_score_bench(nct_ctx* ctx, const int16_t* d_q, int cells, int C, const int16_t* d_seeds_in, int n_in, const int16_t* d_seeds_out, int n_out, int sharpness,
                           int floor_permille, uint8_t* d_score_out, int reps, float* kernel_ms);
/* the re-find kernel alone (SPEC §6.17 rules R1-R3; scripts/region_refind_times.py): nct_region_refind_dev's arguments; one warm-up launch, then `reps` launches
 * (1 … 1000) between two HIP events on the library's own stream; kernel_ms receives the mean device time of one launch. Synchronous. */
int nct_region_refind_bench(nct_ctx* ctx, const uint8_t* d_score, int ht, int wt, const uint8_t* d_prior, int H, int W, int margin, uint8_t* d_out, int reps, float* kernel_ms);
/* the match of reference libraries alone (SPEC §6.21 rule D3; scripts/reflib_times.py): nct_descriptor_match_dev's arguments; one warm-up, then `reps` times (1 … 1000)
 * its three launches (the fill of the column maxima, the match, the sums) between two HIP events on the library's own stream; kernel_ms receives the mean device time
 * of one. Synchronous. */
int nct_descriptor_match_bench(nct_ctx* ctx, const int8_t* d_a, int na, int C, const int8_t* d_rows, const int32_t* offsets, int N, int64_t* d_fwd, int64_t* d_bwd, int reps,
                               float* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* NCT_H */
