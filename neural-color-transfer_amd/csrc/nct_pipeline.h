// nct_pipeline.h — what the pair / multi-reference run (nct_pipeline.cpp) and the frame sequences (nct_seq.cpp) share: the state, the frame setup, the finish of a level.
#pragma once
#include "nct_internal.h"
#include <chrono>
// the last level's finish on a source larger than the working size (SPEC §6.1, §6.9): the original source on the device, H x W, where its result goes, and the finish —
// NCT_FINISH_EXACT moves U1 / S2 / A1 there, NCT_FINISH_UPSAMPLE leaves them at the working size and upsamples S2's output (SPEC §6.8)
// mask (nullable): the source's region mask at H x W, on the device — the exact finish composes with it (SPEC §6.11 rule 5), the upsampling finish of a masked
// sequence frame runs its masked form with it (SPEC §6.13 rule 4)
struct full_target { const uint8_t* src = nullptr; int H = 0, W = 0; uint8_t* out = nullptr; int finish = NCT_FINISH_EXACT; const uint8_t* mask = nullptr; };

// An open frame sequence (SPEC §6.3): what nct_seq_begin prepares once and every frame borrows — the reference's pyramid and its five un-normalised taps (HWC, by
// level) — and the state the blend carries from frame to frame, per level X' ([2][h*w][3] doubles) and L (the frame's level image in 8-bit Lab). All of it comes from
// the context's arena and outlives the runs; the frame and the reference at working size are pair_state's src / ref[0] as for a pair.
// Every block of the two states has one owner, a DevBuf member: it goes back where the member is reset, and with the state (seq_free, nct_pair_free — which
// nct_destroy calls before the arena's blocks are freed). Blocks that change places (X' and warp_x, the kept pull and pull_alt, the matte and matte_alt) swap owners.
// While motion compensation is on (SPEC §6.4, nct_seq_set_motion) it also holds, per level, L packed one word per pixel and the level's field (4 B per level pixel each).
// A propagated frame (SPEC §6.5) with motion on warps X' out of place: warp_x, one map of the largest level run, reserved by the first such frame.
// A sequence over several references (SPEC §6.18, nct_seq_begin_multi) holds the pyramid and the taps once per reference and, per level run, the label map of the last
// frame (1 B per level pixel); a sequence over one reference holds exactly what it always did.
// The two counters of the key-frame decision (SPEC §6.7 rule 3) are host integers: they cost no device memory.
// A full-resolution sequence (SPEC §6.9, nct_seq_begin_fullres) keeps all of that on the working-size grids and adds the frame at its original size H0 x W0 and
// its result: pair_state's full_src / full_out, which live as long as the sequence and are what nct_pair_fit_lut reads; `full` describes them, H = 0 in any other sequence.
// Region tracking (SPEC §6.14, nct_seq_set_region_tracking): the matte in force (pair_state's mask, or full_mask in a full-resolution sequence) is carried out of
// place into matte_alt, a second block of the size frames arrive, reserved by the first carry; then the two change places. The flags and the age are host values.
// Matte snapping (SPEC §6.15, nct_seq_set_region_snap): behind the carry the matte is snapped to the frame's Lab image, again out of place into matte_alt — the block
// the carry has just left — and the two change places once more; a frame that snaps without a carry (motion off) reserves the block the same way.
// Correspondence carry (SPEC §6.23, nct_seq_set_carry): while it is on the sequence also holds, per reference and level run, the two final NNFs of the last full frame
// (4 B per source and per reference level pixel), one forward map and one scratch field of the largest level run; a sequence that never turns it on holds none of it.
struct seq_state {
    nct_params prm; double tau = 0, sigma = 0;
    long frames = 0;                                           // frames since nct_seq_begin / nct_seq_reset: 0 = the next one is a first frame
    long gap = 0;                                              // propagated frames since the last full frame, whichever call ran them
    unsigned long long acc = 0;                                // sum of `changed` over the frames nct_seq_frame_auto propagated since the last full frame
    int ah[5], aw[5], bh[NCT_MAX_REFS][5], bw[NCT_MAX_REFS][5];
    DevBuf<uint8_t> rpyr[NCT_MAX_REFS][4]; DevBuf<float> rfeat[NCT_MAX_REFS][5];     // per reference (SPEC §6.18): nct_seq_begin is the list of one
    DevBuf<double> keep_x[5]; DevBuf<uint8_t> keep_lab[5];
    double hold = 0;                                           // SPEC §6.18: the held selection's margin per window tap; plays no part with one reference
    DevBuf<uint8_t> keep_label[5];                             // several references only: the label map l_t of every level run, one byte per level pixel
    bool motion = false; nct_seq_motion mp = {0, 0, 0};
    DevBuf<uint32_t> keep_pk[5]; DevBuf<int16_t> field[5];
    DevBuf<double> warp_x;
    bool tracking = false;                                     // SPEC §6.14: carry the matte along the field in front of every frame but the matte's own
    bool matte_fresh = false;                                  // nct_seq_set_region gave a matte that no frame has used yet: the next frame that runs is its own
    long matte_age = 0;                                        // frames run since the matte's own frame while tracking was on
    DevBuf<uint8_t> matte_alt;
    bool snap = false; nct_region_snap_params snap_p = {0, 0, 0};  // SPEC §6.15: snap the carried matte to the frame's edges with these parameters
    // SPEC §6.17 (nct_seq_set_region_model): the model's rows on the device, [model_n_in + model_n_out][model_C], inside first, held until the model is replaced or removed
    // or the sequence ends; null: no model. model_p: the parameters of the re-find, model_protect: nct_region_params.protect of the re-found matte
    DevBuf<int16_t> model_rows; int model_tap = 0, model_C = 0, model_n_in = 0, model_n_out = 0;
    nct_region_refind_params model_p = {0, 0, 0, 0, {0, 0, 0}}; int model_protect = 0;
    // SPEC §6.19 (nct_seq_set_ref_region): the masked references' level masks Q_k,l below the working size (Q_k at the working size is pair_state's rmask[k]), built once
    // per set call; per level run the held pull P' of the last frame and the block the next hold or carry writes — the rule gathers, so the two change places; pull_kept:
    // keep_pull holds a full frame's P' under the masks in force (false after any set, replace or remove). rh0 / rw0: the references' sizes as they arrived
    DevBuf<uint8_t> rq[NCT_MAX_REFS][4], keep_pull[5], pull_alt[5];
    bool pull_kept = false;
    int rh0[NCT_MAX_REFS] = {}, rw0[NCT_MAX_REFS] = {};
    // SPEC §6.23 (nct_seq_set_carry): per reference and level run the final fields of the last full frame, moved along every later frame's field — A on the source's
    // level grid, B on the reference's; the forward map of the level's field and one scratch field (the moves gather), both of the largest level run. All reserved
    // when the carry is turned on and given back when it is turned off. carry_kept: the fields hold a full frame's result (false before the first one and after
    // nct_seq_reset, a cut or a failed frame). carry_iters: PatchMatch iterations of a frame that merged, -1 = prm.pm_iters
    bool carry = false, carry_kept = false; int carry_iters = -1;
    DevBuf<uint32_t> keep_ann[NCT_MAX_REFS][5], keep_bnn[NCT_MAX_REFS][5], carry_fwd, carry_tmp;
    full_target full;
    const full_target* target() const { return full.H ? &full : nullptr; }
};
struct pair_state {
    DevBuf<uint8_t> src, out;                                  // device BGR images
    seq_state* seq = nullptr;
    DevBuf<uint8_t> ref[NCT_MAX_REFS];                         // the K references (SPEC §6.2; a pair: K = 1)
    int K = 0;
    int sh = 0, sw = 0, rh[NCT_MAX_REFS] = {}, rw[NCT_MAX_REFS] = {};
    DevBuf<uint8_t> full_src, full_out;                        // a finished full-resolution run (SPEC §6.1): the original source and its result, full_h x full_w, kept for nct_pair_fit_lut
    int full_h = 0, full_w = 0;
    DevBuf<uint8_t> mask, full_mask;                           // the source's region mask (SPEC §6.11): sh x sw bytes, set by nct_pair_set_region, dropped with the images; after a masked
    int protect = 0;                                           // full-resolution run also the mask at full_h x full_w, beside full_src / full_out. protect: nct_region_params
                                                               // An open sequence (SPEC §6.13): both are nct_seq_set_region's and go back with the sequence (seq_free)
    DevBuf<uint8_t> rmask[NCT_MAX_REFS];                       // the references' region masks (SPEC §6.12): rh[k] x rw[k] bytes, set by nct_pair_set_ref_region, dropped with the images
                                                               // An open sequence (SPEC §6.19): nct_seq_set_ref_region's, at the references' working size
    DevBuf<uint8_t> fin_mask;                                  // the last level's target mask F of a run with a reference mask, at the size of its result (rule 7: nct_pair_fit_lut); gone with the next run
    bool ref_masked() const { for (const DevBuf<uint8_t>& m : rmask) if (m.ok()) return true; return false; }
    bool finished = false;                                     // the last run on these images ran to its end: `out` (or full_out) holds its result
};

// a source-masked run's report (SPEC §6.11, §6.13) is the part of the reference-masked one's that it has: M_l and X'
NCT_LOCAL nct_ref_region_levels ref_region_levels_of(const nct_region_levels& levels);
static const int kTapC[5] = {64, 128, 256, 512, 512};       // tap 1 (conv1_1) … tap 5 (conv5_1)
#define MARK(stage, level) NCT_TRY(ctx->mark(s, nct_stage_tag(stage, level)))

// ---- nct_pipeline.cpp
NCT_LOCAL pair_state* pair_of(nct_ctx* ctx);
NCT_LOCAL void drop_images(pair_state* P);                  // drop what the context holds of the last pair / reference list
// what a run is asked for beside its result, every member nullable and filled by name (run_extras x; x.fin = …;). lv: host copies of the level intermediates; color (a pair
// only): [5] the colour stage's coefficient maps per level; fin (K = 1, or a frame of a sequence): the full-resolution finish; seq: the run is a frame of this open sequence, slv: where that
// frame's X'_t, tau_p and fields go; qlv: where a masked run reports Q_k,l, P_k,l, M_l, F_l and X' (SPEC §6.11, §6.12: the one report target of both kinds of mask);
// refusal: the entry point asked for the report of a mask that is not set — the run is refused with NCT_ERR_STATE and this text, behind the checks of state and parameters
// hlv: where a frame of a sequence over several references reports the held selection's free labels and margins (SPEC §6.18)
// plv: where a frame of a sequence with a reference mask reports the merged pull before and after its hold (SPEC §6.19)
struct run_extras { const nct_multi_levels* lv = nullptr; const nct_color_stages* const* color = nullptr; const full_target* fin = nullptr; seq_state* seq = nullptr;
                    const nct_seq_levels* slv = nullptr; const nct_ref_region_levels* qlv = nullptr; const char* refusal = nullptr; const nct_seq_hold_levels* hlv = nullptr;
                    const nct_seq_pull_levels* plv = nullptr; };
// run the whole L=5->1 loop on the uploaded source and its K references
NCT_LOCAL int process_resident(nct_ctx* ctx, const nct_params* prm, nct_pair_timing* timing, const run_extras& x = {});
// a pair is the list of one reference (SPEC §6.2): its maps are reference 0's NNFs and the merged guide / err; it has no label map and no G_k / E_k of their own
NCT_LOCAL nct_multi_levels multi_levels_of(const nct_pair_levels& levels);
// the bracket around a timed run: the constructor clears `timing` (nullable) and switches the stage marks and the kernel clock on as the flags ask; stop() switches them
// off, whatever became of the run; read(), after a run that succeeded and was synchronised, fills `timing`
struct run_clock {
    nct_ctx* const ctx; nct_pair_timing* const timing; const std::chrono::steady_clock::time_point wall0;
    NCT_LOCAL run_clock(nct_ctx* c, nct_pair_timing* t, int flags);
    void stop() { ctx->tm_on = false; ctx->kt_on = false; }
    NCT_LOCAL int read(bool count);
};
// level geometry, coarse -> fine (level 0 = conv5_1): four ceil-halvings of h x w
static inline void level_sizes(int h, int w, int* lh, int* lw) {
    for (int t = 0; t < 5; ++t) { lh[4 - t] = h; lw[4 - t] = w; h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
}
// level l of one image's pyramid (main.cu:104-108): a block of its own, resized from level l + 1; img[l] then names it
static inline int pyramid_level(nct_ctx* ctx, hipStream_t s, DevBuf<uint8_t>& buf, const uint8_t** img, const int* lh, const int* lw, int l) {
    if (!buf.alloc(ctx, (size_t)lh[l] * lw[l] * 3)) return NCT_ERR_HIP;
    NCT_TRY(nctk_resize_u8c3(ctx, s, img[l + 1], lh[l + 1], lw[l + 1], buf, lh[l], lw[l]));
    img[l] = buf;
    return NCT_OK;
}
// an image the caller holds at h0 x w0 onto the device as dst (h x w): uploaded at its own size and shrunk there (SPEC §6.1 rule 1: nct_resize_u8c3's arithmetic).
// at0 (nullable): where the original goes and stays; null: scratch, back in the arena once the resize is enqueued
static inline int upload_shrunk(nct_ctx* ctx, const uint8_t* host, int h0, int w0, uint8_t* dst, int h, int w, uint8_t* at0 = nullptr) {
    DevBuf<uint8_t> scratch;
    if (!at0) { if (!scratch.alloc(ctx, (size_t)h0 * w0 * 3)) return NCT_ERR_HIP; at0 = scratch; }
    NCT_H2D(at0, host, (size_t)h0 * w0 * 3);
    return nctk_resize_u8c3(ctx, ctx->stream, at0, h0, w0, dst, h, w);
}
// The exact finish's two Lab images at full->H x full->W, scratch of the run: open() reserves them and converts the source, and is a no-op for any other finish. A step
// of its own: a level that runs its colour solve enqueues it BEFORE T1, a propagated frame right before the finish (the order of launches and arena requests)
struct NCT_LOCAL full_lab {
    DevBuf<uint8_t> s0, out0;
    NCT_LOCAL int open(nct_ctx* ctx, hipStream_t s, const full_target* full);
};
// The finish of a level: U1 / S2 / A1 of x ([2][h*w][3], the level grid) and the result in BGR. full == null (every level but a full-resolution run's last): onto the
// working grid H x W, s_lab_full -> out_lab -> out_bgr. The exact finish: onto the original source through fl's images into full->out; out_lab and out_bgr stay as they
// are. The upsampling finish (SPEC §6.8): the working-size finish, and behind it S2's output upsampled onto the original source into full->out
// region (nullable; SPEC §6.11 rule 3, §6.12 rule 5): the run is masked — the compose with the source takes the place of Lab -> BGR. mask: the compose mask at the size this
// finish targets (the exact finish: full's size, and the source is full's; else H x W and s_bgr). The upsampling finish of a masked run (SPEC §6.13 rule 4) composes at
// H x W with `mask` and on the original source with full->mask, in the upsampling pass itself
struct region_fin { const uint8_t* mask; const uint8_t* s_bgr; int protect; };
NCT_LOCAL int finish_level(nct_ctx* ctx, hipStream_t s, const double* x, int h, int w, int H, int W, const uint8_t* s_lab_full, uint8_t* out_lab, uint8_t* out_bgr,
                           const full_target* full, const full_lab& fl, const nct_color_params& cp, const nct_color_debug* dbg, int cube, const region_fin* region = nullptr);
// The finish of a masked level, the one copy of SPEC §6.11 rule 3, §6.12 rules 4-5, §6.13 rules 2-4 and §6.19 rule 8, for a level of a run and for a propagated frame:
// the mix mask M_l, the compose mask F_l at the size the finish targets, the mix of x_from by M_l into x_mix, finish_level on the mixed map. Without a reference mask
// (p_l null) M_l is the source's level mask and F_l the source's mask as it came: no launch but the mix. With one, M_l = min(p_l, mask_l) — made here unless the caller
// has made it (m_l) — and F_l = min(resize(p_l), the source's mask at that size); the masked upsampling finish also composes on the original with
// F0 = min(resize(p_l -> full's size), full->mask), through a copy of the target that names it. F of the last level has the size of the result and is kept as fin_mask
// for nct_pair_fit_lut (the masked upsampling finish: F0). The owners are filled here where they are empty, in the order m_buf, f_buf or fin_mask, fin_mask (F0), x_mix:
// a level of a run brings m_buf, f_buf and x_mix from its own requests, a propagated frame brings them empty. The other arguments are finish_level's
struct masked_fin {
    const uint8_t* p_l;                            // P_l, or a propagated frame's P', on the level grid; null: no reference mask
    const uint8_t *mask_l, *mask_work;             // the source's mask on the level grid and at H x W; null: no source mask. At the target's size it is full->mask
    const uint8_t* s_bgr; int protect;             // the source at H x W and nct_region_params.protect: what the compose reads
    bool last;                                     // the run's last level: its F is kept
    const uint8_t* m_l;                            // in: M_l where the caller has made it, else null; out: the mix mask, h x w
    const uint8_t* f_l = nullptr; int fh = 0, fw = 0;   // out: the compose mask and its size, for the caller's report
};
NCT_LOCAL int finish_level_masked(nct_ctx* ctx, hipStream_t s, masked_fin& mf, const double* x_from, DevBuf<double>& x_mix, DevBuf<uint8_t>& m_buf, DevBuf<uint8_t>& f_buf,
                                  DevBuf<uint8_t>& fin_mask, int h, int w, int H, int W, const uint8_t* s_lab_full, uint8_t* out_lab, uint8_t* out_bgr, const full_target* full,
                                  const full_lab& fl, const nct_color_params& cp, const nct_color_debug* dbg, int cube);
// SPEC §6.11 rule 1: a source mask's level masks from level 3 down to level `down_to`, each a block of its own resized from the level above like the image pyramid;
// mimg[4] is the mask at the working size, mimg[l] then names level l's
static inline int source_mask_levels(nct_ctx* ctx, hipStream_t s, DevBuf<uint8_t>* mpyr, const uint8_t** mimg, const int* lh, const int* lw, int down_to) {
    for (int l = 3; l >= down_to; --l) {
        if (!mpyr[l].alloc(ctx, (size_t)lh[l] * lw[l])) return NCT_ERR_HIP;
        NCT_TRY(nctk_resize_u8c1(ctx, s, mimg[l + 1], lh[l + 1], lw[l + 1], mpyr[l], lh[l], lw[l]));
        mimg[l] = mpyr[l];
    }
    return NCT_OK;
}
// the first lines of what acts on the open sequence: P names the context's pair state, refused without one
#define NCT_OPEN_SEQ(P, who) pair_state* const P = (pair_state*)ctx->pair; \
    if (!P || !P->seq) return ctx->fail(NCT_ERR_STATE, "%s: no sequence is open (nct_seq_begin first)", who)
// nct_pair_set_region with the mask already on the device (nct_pair_select_region, SPEC §6.16): the same checks, block and state, a device-to-device copy
NCT_LOCAL int pair_set_region_dev(nct_ctx* ctx, const uint8_t* d_mask, const nct_region_params* region);
// ---- nct_region_select.cpp, shared with the region models of nct_region_model.cpp (SPEC §6.17)
// the argument checks of nct_region_select[_dev] (`who` names the entry point in the message); on success *p holds the parameters in force
NCT_LOCAL int select_check(nct_ctx* ctx, const char* who, const void* src_bgr, int h, int w, const void* strokes, const nct_region_select_params* params, const void* mask_out,
                           nct_region_select_params* p);
// SPEC §6.16 rules 1 and 2 on a device image: the quantised rows of tap `tap`, [cells][C], into the caller's q
NCT_LOCAL int select_quantised_tap(nct_ctx* ctx, hipStream_t s, const uint8_t* d_src, int h, int w, int tap, int16_t* q);
// what rules 1-3 leave on the device, in the order the blocks are requested: the rows, rule 3's flags and scan, the cell codes, rule 4's scores (requested only where
// the caller runs rule 4), the kept seeds' cells and their rows [k_in + k_out][C], inside first
struct select_rows { DevBuf<int16_t> q; DevBuf<unsigned> flags; DevBuf<unsigned long long> pre; DevBuf<uint8_t> code, m; DevBuf<int> idx; DevBuf<int16_t> seeds; unsigned k_in = 0, k_out = 0; };
NCT_LOCAL int select_seed_rows(nct_ctx* ctx, const char* who, const uint8_t* d_src, int h, int w, const uint8_t* d_strokes, const nct_region_select_params& p,
                               const nct_region_select_stages* st, bool with_m, select_rows& r);
// ---- nct_seq.cpp
// nct_seq_set_region with the mask already on the device, at the size frames arrive (nct_seq_select_region, SPEC §6.16)
NCT_LOCAL int seq_set_region_dev(nct_ctx* ctx, const uint8_t* d_mask, const nct_region_params* region);
NCT_LOCAL void seq_free(pair_state* P);                     // what an open sequence holds goes back to the arena, its region mask included
// SPEC §6.4: level l's field from L_t (`lab`) and the kept packed map: the first level run searches radius0 around (0, 0), every other level radius around twice the
// previous level's vector
NCT_LOCAL int seq_motion_level(nct_ctx* ctx, hipStream_t s, seq_state* q, int l, const uint8_t* lab);
// The chain ahead of the expensive stages, shared by the probe (SPEC §6.7 rule 2) and the carry of a full frame (SPEC §6.14): for l = 0 … top the frame's level image
// simg[l] in Lab into lab[l] (requested here, the caller's to give back) and, with motion on, level l's field against the kept packed map into the level's field buffer
NCT_LOCAL int seq_field_chain(nct_ctx* ctx, hipStream_t s, seq_state* q, const uint8_t* const* simg, int top, DevBuf<uint8_t>* lab);
// SPEC §6.14 rule 2, in front of a frame's level masks: nothing without a matte; the matte's own frame only marks it used; else, with tracking on, the age counts and —
// where the frame has a field (motion on, a sequence with state) — the matte is carried through the field of the top level run, the two blocks change places, and a
// full-resolution sequence shrinks the carried matte to the working size. simg: the frame's pyramid, from which a full frame finds the fields first; null: a
// propagated frame, whose level loop has just left them in the field buffers. With snapping on (SPEC §6.15) a sequence with state then snaps the matte, carried or
// not, to the frame's Lab image at the size frames arrive: lab_work, the working-size frame in Lab that the caller holds, or — a full-resolution sequence whose
// frames are larger — the original frame converted into scratch of this call
NCT_LOCAL int seq_track_step(nct_ctx* ctx, hipStream_t s, pair_state* P, seq_state* q, const uint8_t* const* simg, const uint8_t* lab_work);
// The tail of the track step and of the re-find (SPEC §6.15 rule 3, §6.17 rule S5): `iters` snap passes of the matte in force against the frame's Lab image at the
// size frames arrive (lab_work, or the original frame converted into scratch of this call), each out of place into matte_alt — reserved by the caller — after which
// the two change places; then a full-resolution sequence shrinks the matte to the working-size one, as nct_seq_set_region makes it
NCT_LOCAL int seq_matte_snap(nct_ctx* ctx, hipStream_t s, pair_state* P, seq_state* q, const uint8_t* lab_work, const nct_region_snap_params& sp, int iters);
// SPEC §6.23 rules 3-5: the kept fields of reference k at level run l follow the level's field q->field[l], which the caller has found — A through the word gather, B
// through the forward map, which is built with k == 0 and serves the level's other references. Each goes through the scratch field and back. Motion off: nothing
NCT_LOCAL int seq_carry_move(nct_ctx* ctx, hipStream_t s, seq_state* q, int l, int k);
static inline int seq_carry_iters(const seq_state* q) { return q->carry_iters < 0 ? q->prm.pm_iters : q->carry_iters; }
// ---- nct_region_model.cpp
// SPEC §6.17 rules S2-S5, behind a full frame's forward and in front of its level masks: the frame's matte re-found from tap_hwc — the model's tap of that forward,
// un-normalised and channel-last on the working-size grid — with the matte the track step left as the prior (none without a matte or without state), straight to the size
// frames arrive, then the model's snap passes with the frame's Lab image at that size (lab_work, or the original frame converted into scratch) and, in a
// full-resolution sequence, the shrink to the working-size matte. A sequence without a matte gets its matte blocks here
NCT_LOCAL int seq_refind_step(nct_ctx* ctx, hipStream_t s, pair_state* P, seq_state* q, const float* tap_hwc, const uint8_t* lab_work);
// A level of a sequence frame (SPEC §6.3), between S1 and the finish: X'_t = the blend of S1's output x with X'_(t-1), into the kept state q->keep_x[l], which the finish
// then reads; L_t (`lab`) replaces L_(t-1). The first frame and tau == 0 only keep the state, with no blend launch. tmap: the caller's, requested here where slv asks
// for the tau_p map and reserved until the finish has been enqueued. slv (nullable): host copies of X'_t, tau_p and the field
// field_found: the level's field is already in q->field[l] — the held selection of a frame over several references (SPEC §6.18) found it in front of itself — and is not searched again
NCT_LOCAL int seq_level_step(nct_ctx* ctx, hipStream_t s, seq_state* q, int l, const uint8_t* lab, double* x, DevBuf<double>& tmap, const nct_seq_levels* slv, bool field_found = false);
