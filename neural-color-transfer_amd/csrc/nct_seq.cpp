// nct_seq.cpp — frame sequences (SPEC §6.3-§6.9, their region mask §6.13, its tracking §6.14, the snap §6.15, several references §6.18, their region masks §6.19 and the correspondence carry §6.23): the state an open sequence keeps in the context's arena, what a level of a frame does between S1 and the finish,
// the frame entry points — a full frame is a run of nct_pipeline.cpp's level loop — the propagated frame, the probe and the key-frame decision.
#include "nct_pipeline.h"
#include <cstring>
#include <algorithm>

// what motion compensation holds goes back to the arena
static void seq_motion_free(seq_state* q) {
    for (int l = 0; l < 5; ++l) { q->keep_pk[l].reset(); q->field[l].reset(); }
    q->warp_x.reset();
    q->motion = false;
}
// the sequence's matte blocks go back to the arena (the caller has waited for the stream)
static void seq_mask_drop(pair_state* P, seq_state* q) {
    P->mask.reset(); P->full_mask.reset(); q->matte_alt.reset();
    q->full.mask = nullptr; P->protect = 0; q->matte_fresh = false; q->matte_age = 0;
}
// what an open sequence holds goes back to the arena: its region mask (SPEC §6.13 rule 1), which lives in the pair state, ends with it; everything else is the
// state's own and goes back with it. The reference masks at the working size go back with the images (drop_images)
void seq_free(pair_state* P) {
    if (!P->seq) return;
    seq_mask_drop(P, P->seq);
    delete P->seq; P->seq = nullptr;
}

int seq_motion_level(nct_ctx* ctx, hipStream_t s, seq_state* q, int l, const uint8_t* lab) {
    return nctk_seq_motion(ctx, s, lab, q->keep_pk[l], q->ah[l], q->aw[l], l > 0 ? q->field[l - 1] : nullptr, l > 0 ? q->ah[l - 1] : 0, l > 0 ? q->aw[l - 1] : 0,
                           l == 0 ? q->mp.radius0 : q->mp.radius, q->mp.penalty, q->field[l]);
}

int seq_level_step(nct_ctx* ctx, hipStream_t s, seq_state* q, int l, const uint8_t* lab, double* x, DevBuf<double>& tmap, const nct_seq_levels* slv, bool field_found) {
    const int h = q->ah[l], w = q->aw[l], n = h * w;
    const bool blend = q->frames > 0 && q->tau > 0.0;
    double* const keep_x = q->keep_x[l];
    if (slv && slv->tau_map[l] && !tmap.alloc(ctx, n)) return NCT_ERR_HIP;
    if (blend && q->motion) {
        // with motion (SPEC §6.4): the level's field, then the blend gathers X'_(t-1) and L_(t-1) through it — not in place: into S1's own buffer, then into the state
        if (!field_found) NCT_TRY(seq_motion_level(ctx, s, q, l, lab));
        NCT_TRY(nctk_seq_blend(ctx, s, x, keep_x, lab, q->keep_lab[l], h, w, q->tau, q->sigma, x, tmap, q->field[l]));
        NCT_HIP(hipMemcpyAsync(keep_x, x, sizeof(double) * (size_t)6 * n, hipMemcpyDeviceToDevice, s));
        if (slv) NCT_TRY(dbg_copy(ctx, s, slv->motion[l], q->field[l], (size_t)2 * n));
    } else if (blend) NCT_TRY(nctk_seq_blend(ctx, s, x, keep_x, lab, q->keep_lab[l], h, w, q->tau, q->sigma, keep_x, tmap));
    else {
        NCT_HIP(hipMemcpyAsync(keep_x, x, sizeof(double) * (size_t)6 * n, hipMemcpyDeviceToDevice, s));
        if (tmap.ok()) NCT_HIP(hipMemsetAsync(tmap, 0, sizeof(double) * (size_t)n, s));
    }
    NCT_HIP(hipMemcpyAsync(q->keep_lab[l], lab, (size_t)3 * n, hipMemcpyDeviceToDevice, s));
    if (q->motion) NCT_TRY(nctk_seq_pack(ctx, s, lab, n, q->keep_pk[l]));
    if (slv) NCT_TRY(dbg_copy(ctx, s, slv->ab_blend[l], keep_x, (size_t)6 * n));
    if (tmap.ok()) NCT_TRY(dbg_copy(ctx, s, slv->tau_map[l], (double*)tmap, n));
    return NCT_OK;
}

// what the correspondence carry holds goes back to the arena (the caller has waited for the stream)
static void seq_carry_free(seq_state* q) {
    for (int k = 0; k < NCT_MAX_REFS; ++k) for (int l = 0; l < 5; ++l) { q->keep_ann[k][l].reset(); q->keep_bnn[k][l].reset(); }
    q->carry_fwd.reset(); q->carry_tmp.reset();
    q->carry = false; q->carry_kept = false; q->carry_iters = -1;
}

int seq_carry_move(nct_ctx* ctx, hipStream_t s, seq_state* q, int l, int k) {
    if (!q->motion) return NCT_OK;                               // m = 0: both moves are the identity and enqueue nothing
    const int h = q->ah[l], w = q->aw[l], bh = q->bh[k][l], bw = q->bw[k][l];
    NCT_TRY(nctk_nnf_carry(ctx, s, q->keep_ann[k][l], h, w, q->field[l], q->carry_tmp));
    NCT_HIP(hipMemcpyAsync(q->keep_ann[k][l], q->carry_tmp, sizeof(uint32_t) * (size_t)h * w, hipMemcpyDeviceToDevice, s));
    if (k == 0) NCT_TRY(nctk_nnf_forward_map(ctx, s, q->field[l], h, w, q->carry_fwd));
    NCT_TRY(nctk_nnf_remap(ctx, s, q->keep_bnn[k][l], bh, bw, q->carry_fwd, h, w, q->carry_tmp));
    NCT_HIP(hipMemcpyAsync(q->keep_bnn[k][l], q->carry_tmp, sizeof(uint32_t) * (size_t)bh * bw, hipMemcpyDeviceToDevice, s));
    return NCT_OK;
}

int seq_field_chain(nct_ctx* ctx, hipStream_t s, seq_state* q, const uint8_t* const* simg, int top, DevBuf<uint8_t>* lab) {
    for (int l = 0; l <= top; ++l) {
        const int h = q->ah[l], w = q->aw[l];
        if (!lab[l].alloc(ctx, (size_t)h * w * 3)) return NCT_ERR_HIP;
        NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], lab[l], (size_t)h * w));
        if (q->motion) NCT_TRY(seq_motion_level(ctx, s, q, l, lab[l]));
    }
    return NCT_OK;
}

int seq_track_step(nct_ctx* ctx, hipStream_t s, pair_state* P, seq_state* q, const uint8_t* const* simg, const uint8_t* lab_work) {
    if (!P->mask) return NCT_OK;
    if (q->matte_fresh) { q->matte_fresh = false; return NCT_OK; }          // the matte's own frame uses it as it came: age 0
    if (!q->tracking) return NCT_OK;
    q->matte_age += 1;
    // a sequence without state (a first frame, a frame after nct_seq_reset, a CUT frame) has a zero field and nothing to snap to: the matte marks a place in a shot
    // that is over. With motion off the field is zero too: the matte stays where it is, and only the snap (SPEC §6.15) may re-fit it
    if (q->frames == 0 || (!q->motion && !q->snap)) return NCT_OK;
    const int top = q->prm.levels - 1;
    if (q->motion && simg) {
        // a full frame finds its fields here, ahead of its level masks, whether or not it blends; the Lab scratch goes back with this call
        DevBuf<uint8_t> lab[5];
        NCT_TRY(seq_field_chain(ctx, s, q, simg, top, lab));
    }
    DevBuf<uint8_t>& matte = q->target() ? P->full_mask : P->mask;
    const int H = q->target() ? q->full.H : P->sh, W = q->target() ? q->full.W : P->sw;
    if (!q->matte_alt.reserve(ctx, (size_t)H * W)) return NCT_ERR_HIP;
    if (q->motion) {
        NCT_TRY(nctk_seq_matte_warp(ctx, s, matte, H, W, q->field[top], q->ah[top], q->aw[top], q->matte_alt));
        matte.swap(q->matte_alt);
    }
    // SPEC §6.15 rule 3: one pass; the block the carry has left takes the snapped matte
    return seq_matte_snap(ctx, s, P, q, lab_work, q->snap_p, q->snap ? 1 : 0);
}

int seq_matte_snap(nct_ctx* ctx, hipStream_t s, pair_state* P, seq_state* q, const uint8_t* lab_work, const nct_region_snap_params& sp, int iters) {
    DevBuf<uint8_t>& matte = q->target() ? P->full_mask : P->mask;
    const int H = q->target() ? q->full.H : P->sh, W = q->target() ? q->full.W : P->sw;
    if (iters > 0) {
        DevBuf<uint8_t> lab0;
        const uint8_t* guide = lab_work;
        if (H != P->sh || W != P->sw) {
            if (!lab0.alloc(ctx, (size_t)H * W * 3)) return NCT_ERR_HIP;
            NCT_TRY(nctk_bgr2lab(ctx, s, P->full_src, lab0, (size_t)H * W));
            guide = lab0;
        }
        for (int it = 0; it < iters; ++it) {
            NCT_TRY(nctk_region_snap(ctx, s, matte, guide, H, W, &sp, q->matte_alt));
            matte.swap(q->matte_alt);
        }
    }
    if (q->target()) {
        // the carry, the re-find and the snap ran at the original size; the working-size matte is the shrink of their result
        q->full.mask = P->full_mask;
        NCT_TRY(nctk_resize_u8c1(ctx, s, P->full_mask, H, W, P->mask, P->sh, P->sw));
    }
    return NCT_OK;
}

extern "C" {

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
    seq_free(P);
    drop_images(P);
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
    NCT_OPEN_SEQ(P, "seq_set_motion");
    seq_state* q = P->seq;
    if (mp) {
        NCT_REQUIRE(mp->radius0 >= 0 && mp->radius0 <= 8, "seq_set_motion: radius0 must be in [0, 8] (got %d)", mp->radius0);
        NCT_REQUIRE(mp->radius >= 0 && mp->radius <= 3, "seq_set_motion: radius must be in [0, 3] (got %d)", mp->radius);
        NCT_REQUIRE(mp->penalty >= 0 && mp->penalty <= 255, "seq_set_motion: penalty must be in [0, 255] (got %d)", mp->penalty);
    }
    const bool on = mp && (mp->radius0 > 0 || mp->radius > 0);
    if (!on) {
        if (q->motion) { NCT_SYNC(); seq_motion_free(q); }
        return NCT_OK;
    }
    q->mp = *mp;
    if (q->motion) return NCT_OK;
    for (int l = 0; l < q->prm.levels; ++l) {
        const size_t n = (size_t)q->ah[l] * q->aw[l];
        if (!q->keep_pk[l].alloc(ctx, n) || !q->field[l].alloc(ctx, 2 * n)) { seq_motion_free(q); return NCT_ERR_HIP; }
    }
    q->motion = true;
    if (q->frames > 0) {
        for (int l = 0; l < q->prm.levels; ++l) {
            const int rc = nctk_seq_pack(ctx, ctx->stream, q->keep_lab[l], q->ah[l] * q->aw[l], q->keep_pk[l]);
            if (rc) { seq_motion_free(q); return rc; }
        }
    }
    return NCT_OK;
}

int nct_seq_reset(nct_ctx* ctx) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_reset");
    P->seq->frames = 0; P->seq->gap = 0; P->seq->acc = 0;
    P->seq->carry_kept = false;                                  // SPEC §6.23 rule 1: the kept fields belong to a shot that is over
    return NCT_OK;
}

// SPEC §6.23: the correspondence carry of the open sequence on (from the next full frame) or off. Turning it on reserves the kept fields of every reference and level
// run, the forward map and the scratch field; turning it off gives them back
int nct_seq_set_carry(nct_ctx* ctx, int on, int iters) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_set_carry");
    NCT_REQUIRE(on == 0 || on == 1, "seq_set_carry: on must be 0 or 1 (got %d)", on);
    NCT_REQUIRE(iters >= -1 && iters <= 64, "seq_set_carry: iters must be in [0, 64], or -1 for the sequence's pm_iters (got %d)", iters);
    seq_state* q = P->seq;
    if (!on) {
        if (q->carry) { NCT_SYNC(); seq_carry_free(q); }
        return NCT_OK;
    }
    if (q->carry) { q->carry_iters = iters; return NCT_OK; }
    size_t big = 0;
    bool ok = true;
    for (int l = 0; l < q->prm.levels && ok; ++l) {
        const size_t n = (size_t)q->ah[l] * q->aw[l];
        big = std::max(big, n);
        for (int k = 0; k < P->K && ok; ++k) {
            const size_t nr = (size_t)q->bh[k][l] * q->bw[k][l];
            big = std::max(big, nr);
            ok = q->keep_ann[k][l].alloc(ctx, n) && q->keep_bnn[k][l].alloc(ctx, nr);
        }
    }
    const int top = q->prm.levels - 1;
    ok = ok && q->carry_fwd.alloc(ctx, (size_t)q->ah[top] * q->aw[top]) && q->carry_tmp.alloc(ctx, big);
    if (!ok) { seq_carry_free(q); return NCT_ERR_HIP; }
    q->carry = true; q->carry_kept = false; q->carry_iters = iters;
    return NCT_OK;
}

int nct_seq_get_carry(nct_ctx* ctx, int k, int l, uint32_t* ann, uint32_t* bnn) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_get_carry");
    const seq_state* q = P->seq;
    NCT_REQUIRE(k >= 0 && k < P->K, "seq_get_carry: k = %d is not one of the sequence's %d references", k, P->K);
    NCT_REQUIRE(l >= 0 && l < q->prm.levels, "seq_get_carry: l = %d is not one of the sequence's %d level runs", l, q->prm.levels);
    if (!q->carry || !q->carry_kept) return ctx->fail(NCT_ERR_STATE, "seq_get_carry: the sequence holds no kept fields (nct_seq_set_carry, then a full frame)");
    if (ann) NCT_D2H(ann, q->keep_ann[k][l], sizeof(uint32_t) * (size_t)q->ah[l] * q->aw[l]);
    if (bnn) NCT_D2H(bnn, q->keep_bnn[k][l], sizeof(uint32_t) * (size_t)q->bh[k][l] * q->bw[k][l]);
    NCT_SYNC();
    return NCT_OK;
}

// the mask of nct_seq_set_region onto the device, into blocks the sequence keeps until the mask is removed: at the size it came, and (a full-resolution sequence) shrunk
static int seq_mask_upload(nct_ctx* ctx, pair_state* P, seq_state* q, const uint8_t* mask, hipMemcpyKind kind) {
    const size_t n = (size_t)P->sh * P->sw;
    if (!P->mask.reserve(ctx, n)) return NCT_ERR_HIP;
    if (q->target()) {
        const size_t n0 = (size_t)q->full.H * q->full.W;
        if (!P->full_mask.reserve(ctx, n0)) return NCT_ERR_HIP;
        NCT_HIP(hipMemcpyAsync(P->full_mask, mask, n0, kind, ctx->stream));
        NCT_TRY(nctk_resize_u8c1(ctx, ctx->stream, P->full_mask, q->full.H, q->full.W, P->mask, P->sh, P->sw));
        q->full.mask = P->full_mask;
    } else NCT_HIP(hipMemcpyAsync(P->mask, mask, n, kind, ctx->stream));
    NCT_SYNC();
    return NCT_OK;
}

// SPEC §6.13 rule 1: the open sequence's region mask, sticky from the next frame on. It arrives at the size frames arrive; a full-resolution sequence keeps it at that
// size (the exact and the upsampling finish compose with it, nct_pair_fit_lut reads it) and shrinks it on the device to the working size. NULL removes it
// kind: where `mask` lives — the caller's memory (nct_seq_set_region) or the device (seq_set_region_dev)
static int seq_set_region_from(nct_ctx* ctx, const uint8_t* mask, const nct_region_params* region, hipMemcpyKind kind) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_set_region");
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "seq_set_region: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    seq_state* q = P->seq;
    // the state stays; what the last frame left is no longer the result of these settings
    P->finished = false;
    if (!mask) {
        if (P->mask.ok() || P->full_mask.ok()) NCT_SYNC();
        seq_mask_drop(P, q);
        return NCT_OK;
    }
    const int rc = seq_mask_upload(ctx, P, q, mask, kind);
    if (rc) {
        // a device error half way: no mask is better than a block of unknown bytes
        (void)hipStreamSynchronize(ctx->stream);
        seq_mask_drop(P, q);
        return rc;
    }
    P->protect = region ? region->protect : 0;
    // SPEC §6.14 rule 2: the matte belongs to the next frame that runs
    q->matte_fresh = true; q->matte_age = 0;
    return NCT_OK;
}
int nct_seq_set_region(nct_ctx* ctx, const uint8_t* mask, const nct_region_params* region) { return seq_set_region_from(ctx, mask, region, hipMemcpyHostToDevice); }

// SPEC §6.14 rule 2: from the next frame on the matte in force follows the motion field (1), or stays where it is as a sticky §6.13 matte (0)
int nct_seq_set_region_tracking(nct_ctx* ctx, int on) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_set_region_tracking");
    NCT_REQUIRE(on == 0 || on == 1, "seq_set_region_tracking: on must be 0 or 1 (got %d)", on);
    P->seq->tracking = on == 1;
    return NCT_OK;
}

// SPEC §6.15 rule 3: from the next frame on a tracked matte is snapped to its frame's edges behind the carry (non-null: with these parameters), or not (null)
int nct_seq_set_region_snap(nct_ctx* ctx, const nct_region_snap_params* params) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_set_region_snap");
    NCT_TRY(nct_region_snap_params_check(ctx, "seq_set_region_snap", params));
    P->seq->snap = params != nullptr;
    if (params) P->seq->snap_p = *params;
    return NCT_OK;
}

// the matte in force at the size frames arrive, and how many frames it has been carried or kept since its own
int nct_seq_get_region(nct_ctx* ctx, uint8_t* mask_out, int* age) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_get_region");
    if (!P->mask) return ctx->fail(NCT_ERR_STATE, "seq_get_region: no region mask is set (nct_seq_set_region first)");
    NCT_REQUIRE(mask_out, "seq_get_region: null mask_out");
    const seq_state* q = P->seq;
    if (q->target()) NCT_D2H(mask_out, P->full_mask, (size_t)q->full.H * q->full.W);
    else NCT_D2H(mask_out, P->mask, (size_t)P->sh * P->sw);
    NCT_SYNC();
    if (age) *age = (int)std::min<long>(q->matte_age, 0x7fffffffL);
    return NCT_OK;
}

// what the sequence holds of reference k's mask goes back to the arena, and with the last mask the kept pull (the caller has waited for the stream)
static void seq_ref_mask_drop(pair_state* P, seq_state* q, int k) {
    P->rmask[k].reset();
    for (int l = 0; l < 4; ++l) q->rq[k][l].reset();
    if (P->ref_masked()) return;
    for (int l = 0; l < 5; ++l) { q->keep_pull[l].reset(); q->pull_alt[l].reset(); }
}

// reference k's mask onto the device at the reference's working size (a full-resolution sequence: uploaded as it came and shrunk there, as its image was), its level
// masks by SPEC §6.12 rule 1 on the reference's level grids, and — with the first mask — the two maps per level run of the kept pull
static int seq_ref_mask_upload(nct_ctx* ctx, pair_state* P, seq_state* q, int k, const uint8_t* mask) {
    const hipStream_t s = ctx->stream;
    if (!P->rmask[k].reserve(ctx, (size_t)P->rh[k] * P->rw[k])) return NCT_ERR_HIP;
    for (int l = 0; l < 4; ++l) if (!q->rq[k][l].reserve(ctx, (size_t)q->bh[k][l] * q->bw[k][l])) return NCT_ERR_HIP;
    for (int l = 0; l < q->prm.levels; ++l) {
        const size_t n = (size_t)q->ah[l] * q->aw[l];
        if (!q->keep_pull[l].reserve(ctx, n) || !q->pull_alt[l].reserve(ctx, n)) return NCT_ERR_HIP;
    }
    if (q->rh0[k] == P->rh[k] && q->rw0[k] == P->rw[k]) NCT_H2D(P->rmask[k], mask, (size_t)P->rh[k] * P->rw[k]);
    else {
        DevBuf<uint8_t> q0(ctx, (size_t)q->rh0[k] * q->rw0[k]);
        if (!q0.ok()) return NCT_ERR_HIP;
        NCT_H2D(q0, mask, (size_t)q->rh0[k] * q->rw0[k]);
        NCT_TRY(nctk_resize_u8c1(ctx, s, q0, q->rh0[k], q->rw0[k], P->rmask[k], P->rh[k], P->rw[k]));
    }
    const uint8_t* img = P->rmask[k];
    for (int l = 3; l >= 0; --l) {
        NCT_TRY(nctk_resize_u8c1(ctx, s, img, q->bh[k][l + 1], q->bw[k][l + 1], q->rq[k][l], q->bh[k][l], q->bw[k][l]));
        img = q->rq[k][l];
    }
    NCT_SYNC();
    return NCT_OK;
}

// SPEC §6.19: reference k's region mask on the open sequence, sticky from the next frame on; NULL removes it. Any call makes the kept pull stale: the next full frame
// keeps its merged pull as it is, and a propagated frame before that is refused
int nct_seq_set_ref_region(nct_ctx* ctx, int k, const uint8_t* mask, const nct_region_params* region) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_set_ref_region");
    NCT_REQUIRE(k >= 0 && k < P->K, "seq_set_ref_region: k = %d is not one of the sequence's %d references", k, P->K);
    NCT_REQUIRE(!region || region->protect == 0 || region->protect == 1, "seq_set_ref_region: region protect must be 0 or 1 (got %d)", region ? region->protect : 0);
    seq_state* q = P->seq;
    // the state stays; what the last frame left is no longer the result of these settings
    P->finished = false;
    q->pull_kept = false;
    NCT_SYNC();
    P->fin_mask.reset();
    if (!mask) seq_ref_mask_drop(P, q, k);
    else {
        const int rc = seq_ref_mask_upload(ctx, P, q, k, mask);
        if (rc) {
            // a device error half way: no mask is better than a block of unknown bytes
            (void)hipStreamSynchronize(ctx->stream);
            seq_ref_mask_drop(P, q, k);
            return rc;
        }
    }
    if (region) P->protect = region->protect;
    return NCT_OK;
}

// the references once, each: upload, pyramid (main.cu:104-108), one VGG19 forward with all five taps kept channel-last; and the per-level state. One reference
// (nct_seq_begin) requests what it always did, in the same order; several (SPEC §6.18) also the label map of every level run
// rh0 x rw0: a reference as the caller holds it — larger than rh x rw only in a full-resolution sequence, which shrinks it on the device (SPEC §6.9)
static int seq_prepare(nct_ctx* ctx, pair_state* P, seq_state* q, int K, const uint8_t* const* refs_bgr, const int* rh0, const int* rw0, const int* rh, const int* rw, int sh, int sw) {
    hipStream_t s = ctx->stream;
    level_sizes(sh, sw, q->ah, q->aw);
    for (int k = 0; k < K; ++k) level_sizes(rh[k], rw[k], q->bh[k], q->bw[k]);
    if (!P->src.alloc(ctx, (size_t)sh * sw * 3)) return NCT_ERR_HIP;
    for (int k = 0; k < K; ++k) if (!P->ref[k].alloc(ctx, (size_t)rh[k] * rw[k] * 3)) return NCT_ERR_HIP;
    P->sh = sh; P->sw = sw; P->K = K;
    for (int k = 0; k < K; ++k) { P->rh[k] = rh[k]; P->rw[k] = rw[k]; q->rh0[k] = rh0[k]; q->rw0[k] = rw0[k]; }
    for (int l = 0; l < 5; ++l) {
        const size_t n = (size_t)q->ah[l] * q->aw[l];
        for (int k = 0; k < K; ++k) {
            const size_t nr = (size_t)q->bh[k][l] * q->bw[k][l];
            if (l < 4 && !q->rpyr[k][l].alloc(ctx, nr * 3)) return NCT_ERR_HIP;
            if (!q->rfeat[k][l].alloc(ctx, kTapC[4 - l] * nr)) return NCT_ERR_HIP;
        }
        if (l < q->prm.levels) {
            if (!q->keep_x[l].alloc(ctx, 6 * n) || !q->keep_lab[l].alloc(ctx, n * 3)) return NCT_ERR_HIP;
            if (K > 1 && !q->keep_label[l].alloc(ctx, n)) return NCT_ERR_HIP;
        }
    }
    for (int k = 0; k < K; ++k) {
        if (rh0[k] == rh[k] && rw0[k] == rw[k]) NCT_H2D(P->ref[k], refs_bgr[k], (size_t)rh[k] * rw[k] * 3);
        else NCT_TRY(upload_shrunk(ctx, refs_bgr[k], rh0[k], rw0[k], P->ref[k], rh[k], rw[k]));
    }
    if (q->target()) {
        if (!P->full_src.alloc(ctx, (size_t)q->full.H * q->full.W * 3) || !P->full_out.alloc(ctx, (size_t)q->full.H * q->full.W * 3)) return NCT_ERR_HIP;
        q->full.src = P->full_src; q->full.out = P->full_out;
        P->full_h = q->full.H; P->full_w = q->full.W;
    }
    for (int k = 0; k < K; ++k) {
        const uint8_t* img = P->ref[k];
        for (int l = 3; l >= 0; --l) {
            NCT_TRY(nctk_resize_u8c3(ctx, s, img, q->bh[k][l + 1], q->bw[k][l + 1], q->rpyr[k][l], q->bh[k][l], q->bw[k][l]));
            img = q->rpyr[k][l];
        }
        float* taps_hwc[5];
        for (int t = 0; t < 5; ++t) taps_hwc[t] = q->rfeat[k][4 - t];
        NCT_TRY(nctk_vgg19_forward(ctx, s, P->ref[k], rh[k], rw[k], rw[k] * 3, 5, nullptr, nullptr, taps_hwc));
    }
    NCT_SYNC();
    return NCT_OK;
}

// what the nct_seq_begin* entry points (`who`) do once the image sizes are settled; full (nullable): the original frame size and the finish of a full-resolution sequence;
// hold (nullable: the default): SPEC §6.18's parameter, which plays no part with one reference
static int seq_open(nct_ctx* ctx, const char* who, int K, const uint8_t* const* refs_bgr, const int* rh0, const int* rw0, const int* rh, const int* rw, int sh, int sw,
                    const full_target* full, const nct_params* prm, const nct_seq_params* sp, const nct_seq_hold* hold) {
    NCT_REQUIRE(sp->tau >= 0.0 && sp->tau < 1.0, "%s: tau must be in [0, 1) (got %g)", who, sp->tau);
    NCT_REQUIRE(sp->sigma > 0.0 && sp->sigma <= 1.7976931348623157e308, "%s: sigma must be finite and positive (got %g)", who, sp->sigma);
    NCT_REQUIRE(prm->levels >= 1 && prm->levels <= 5, "%s: levels must be in [1, 5] (got %d)", who, prm->levels);
    NCT_TRY(nct_params_check(ctx, who, *prm));
    nct_seq_hold hp;
    if (hold) hp = *hold; else nct_seq_hold_default(&hp);
    NCT_REQUIRE(nct_seq_hold_ok(hp.hold), "%s: hold must be finite and in [0, 2] (got %g)", who, hp.hold);
    NCT_TRY(nct_seq_end(ctx));                                   // a sequence that is still open is closed first
    pair_state* P = pair_of(ctx);
    drop_images(P);
    seq_state* q = new seq_state();
    q->prm = *prm; q->tau = sp->tau; q->sigma = sp->sigma; q->hold = hp.hold;
    if (full) q->full = *full;
    P->seq = q;
    const int rc = seq_prepare(ctx, P, q, K, refs_bgr, rh0, rw0, rh, rw, sh, sw);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); seq_free(P); drop_images(P); }
    return rc;
}

int nct_seq_begin(nct_ctx* ctx, const uint8_t* ref_bgr, int rh, int rw, int sh, int sw, const nct_params* prm, const nct_seq_params* sp) {
    NCT_CTX_ENTER();
    NCT_REQUIRE(ref_bgr && prm && sp, "seq_begin: null pointer");
    NCT_REQUIRE(sh >= 17 && sw >= 17 && rh >= 17 && rw >= 17 && sh <= 4000 && sw <= 4000 && rh <= 4000 && rw <= 4000,
                "seq_begin: image sides must be in [17, 4000] (got frames of %dx%d and a reference of %dx%d)", sw, sh, rw, rh);
    return seq_open(ctx, "seq_begin", 1, &ref_bgr, &rh, &rw, &rh, &rw, sh, sw, nullptr, prm, sp, nullptr);
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
    const full_target full{nullptr, sh, sw, nullptr, finish};    // the two images: seq_prepare
    return seq_open(ctx, "seq_begin_fullres", 1, &ref_bgr, &rh, &rw, &rwh, &rww, wh, ww, &full, prm, sp, nullptr);
}

// SPEC §6.18: the same over K references; the list's own checks, then seq_open
void nct_seq_hold_default(nct_seq_hold* p) {
    if (!p) return;
    p->hold = 0.005;
}

static int seq_multi_list_check(nct_ctx* ctx, const char* who, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, const nct_params* prm, const nct_seq_params* sp) {
    NCT_REQUIRE(K >= 1 && K <= NCT_MAX_REFS, "%s: K must be in [1, %d] (got %d)", who, NCT_MAX_REFS, K);
    NCT_REQUIRE(refs_bgr && rh && rw && prm && sp, "%s: null pointer", who);
    for (int k = 0; k < K; ++k) NCT_REQUIRE(refs_bgr[k], "%s: reference %d is null", who, k);
    return NCT_OK;
}

int nct_seq_begin_multi(nct_ctx* ctx, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, int sh, int sw, const nct_params* prm, const nct_seq_params* sp,
                        const nct_seq_hold* hold) {
    NCT_CTX_ENTER();
    NCT_TRY(seq_multi_list_check(ctx, "seq_begin_multi", K, refs_bgr, rh, rw, prm, sp));
    NCT_REQUIRE(sh >= 17 && sw >= 17 && sh <= 4000 && sw <= 4000, "seq_begin_multi: image sides must be in [17, 4000] (got frames of %dx%d)", sw, sh);
    for (int k = 0; k < K; ++k)
        NCT_REQUIRE(rh[k] >= 17 && rw[k] >= 17 && rh[k] <= 4000 && rw[k] <= 4000, "seq_begin_multi: image sides must be in [17, 4000] (got reference %d of %dx%d)", k, rw[k], rh[k]);
    return seq_open(ctx, "seq_begin_multi", K, refs_bgr, rh, rw, rh, rw, sh, sw, nullptr, prm, sp, hold);
}

int nct_seq_begin_multi_fullres(nct_ctx* ctx, int K, const uint8_t* const* refs_bgr, const int* rh, const int* rw, int sh, int sw, int max_side, int finish,
                                const nct_params* prm, const nct_seq_params* sp, const nct_seq_hold* hold) {
    NCT_CTX_ENTER();
    NCT_TRY(seq_multi_list_check(ctx, "seq_begin_multi_fullres", K, refs_bgr, rh, rw, prm, sp));
    NCT_REQUIRE(finish == NCT_FINISH_EXACT || finish == NCT_FINISH_UPSAMPLE, "seq_begin_multi_fullres: finish must be NCT_FINISH_EXACT (0) or NCT_FINISH_UPSAMPLE (1) (got %d)", finish);
    int wh = 0, ww = 0, rwh[NCT_MAX_REFS], rww[NCT_MAX_REFS];
    const char* why = nct_working_size_rule(sh, sw, max_side, &wh, &ww);
    if (why) return ctx->fail(NCT_ERR_INVALID, "seq_begin_multi_fullres: frames of %dx%d, max_side %d: %s", sw, sh, max_side, why);
    for (int k = 0; k < K; ++k) {
        why = nct_working_size_rule(rh[k], rw[k], max_side, &rwh[k], &rww[k]);
        if (why) return ctx->fail(NCT_ERR_INVALID, "seq_begin_multi_fullres: reference %d of %dx%d, max_side %d: %s", k, rw[k], rh[k], max_side, why);
    }
    const full_target full{nullptr, sh, sw, nullptr, finish};    // the two images: seq_prepare
    return seq_open(ctx, "seq_begin_multi_fullres", K, refs_bgr, rh, rw, rwh, rww, wh, ww, &full, prm, sp, hold);
}

// a frame of the open sequence onto the device: into P->src, or (SPEC §6.9) at its original size into full_src and from there shrunk into P->src
static int seq_upload_frame(nct_ctx* ctx, pair_state* P, seq_state* q, const uint8_t* src_bgr) {
    if (!q->target()) { NCT_H2D(P->src, src_bgr, (size_t)P->sh * P->sw * 3); return NCT_OK; }
    return upload_shrunk(ctx, src_bgr, q->full.H, q->full.W, P->src, P->sh, P->sw, P->full_src);
}

// A full frame of the open sequence, the body of every nct_seq_frame*_levels form. mlv (nullable): the level report — a pair's (as_pair: it came as nct_pair_levels, which
// describes one reference) or the list's; color (nullable): the colour stage's maps; hold_levels (nullable; SPEC §6.18): the held selection's report;
// ref_region_levels, pull_levels (nullable; SPEC §6.19): the report of a frame with a reference mask, refused without one
static int seq_frame_run(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* mlv, const nct_color_stages* const* color,
                         bool as_pair, const nct_seq_levels* seq_levels, const nct_region_levels* region_levels, const nct_seq_hold_levels* hold_levels,
                         const nct_ref_region_levels* ref_region_levels = nullptr, const nct_seq_pull_levels* pull_levels = nullptr) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_frame");
    NCT_REQUIRE(src_bgr && out_bgr, "seq_frame: null image");
    seq_state* q = P->seq;
    NCT_REQUIRE(!(q->target() && as_pair), "seq_frame_levels: levels must be NULL in a full-resolution sequence (its result[] arrays have no single size); seq_levels reports the working-size maps");
    NCT_REQUIRE(!(as_pair && P->K > 1), "seq_frame_levels: nct_pair_levels describes a pair; a sequence over several references reports through nct_seq_frame_multi_levels");
    if (q->target() && mlv) for (int l = 0; l < 5; ++l)
        NCT_REQUIRE(!mlv->result[l], "seq_frame_multi_levels: levels->result[] must be NULL in a full-resolution sequence (the arrays have no single size)");
    NCT_REQUIRE(!(q->target() && color), "seq_frame_multi_stage_levels: color must be NULL in a full-resolution sequence");
    // a level without a field (motion off, a first frame, tau == 0) reports zeros
    if (seq_levels) for (int l = 0; l < q->prm.levels; ++l) if (seq_levels->motion[l]) memset(seq_levels->motion[l], 0, sizeof(int16_t) * 2 * (size_t)q->ah[l] * q->aw[l]);
    int rc = seq_upload_frame(ctx, P, q, src_bgr);
    run_extras x; x.fin = q->target(); x.seq = q; x.slv = seq_levels; x.lv = mlv; x.color = color; x.hlv = hold_levels;
    nct_ref_region_levels qlv;
    if (region_levels) { qlv = ref_region_levels_of(*region_levels); x.qlv = &qlv; }
    if (region_levels && !P->mask.ok() && !q->model_rows.ok()) x.refusal = "seq_frame: region levels asked for, but no region mask is set (nct_seq_set_region first)";
    if (ref_region_levels) x.qlv = ref_region_levels;
    x.plv = pull_levels;
    if ((ref_region_levels || pull_levels) && !P->ref_masked()) x.refusal = "seq_frame: reference region levels asked for, but no reference mask is set (nct_seq_set_ref_region first)";
    if (rc == NCT_OK) rc = process_resident(ctx, &q->prm, timing, x);
    // a frame that failed may have replaced the state of some levels only: the next frame starts over
    q->gap = 0; q->acc = 0;                                      // a full frame (and a failed one: the next is a first frame) starts the count over
    if (rc) { q->frames = 0; q->carry_kept = false; return rc; }
    q->frames += 1;
    q->carry_kept = q->carry;                                    // SPEC §6.23 rule 1: every level run now keeps this frame's final fields
    q->pull_kept = P->ref_masked();                              // SPEC §6.19: every level run now keeps this frame's P'
    if (!q->target()) return nct_pair_download(ctx, out_bgr);
    NCT_D2H(out_bgr, P->full_out, (size_t)q->full.H * q->full.W * 3);
    NCT_SYNC();
    return NCT_OK;
}

int nct_seq_frame_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_seq_levels* seq_levels) {
    return nct_seq_frame_region_levels(ctx, src_bgr, out_bgr, timing, levels, seq_levels, nullptr);
}

// region_levels (nullable; SPEC §6.13): where a masked frame's mixed maps and level masks go
int nct_seq_frame_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_pair_levels* levels, const nct_seq_levels* seq_levels,
                                const nct_region_levels* region_levels) {
    if (!levels) return seq_frame_run(ctx, src_bgr, out_bgr, timing, nullptr, nullptr, false, seq_levels, region_levels, nullptr);
    const nct_multi_levels m = multi_levels_of(*levels);
    return seq_frame_run(ctx, src_bgr, out_bgr, timing, &m, levels->color, true, seq_levels, region_levels, nullptr);
}

int nct_seq_frame_multi_stage_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* levels,
                                     const nct_color_stages* const* color, const nct_seq_levels* seq_levels, const nct_seq_hold_levels* hold_levels) {
    return seq_frame_run(ctx, src_bgr, out_bgr, timing, levels, color, false, seq_levels, nullptr, hold_levels);
}

int nct_seq_frame_multi_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* levels, const nct_seq_levels* seq_levels,
                               const nct_seq_hold_levels* hold_levels) {
    return seq_frame_run(ctx, src_bgr, out_bgr, timing, levels, nullptr, false, seq_levels, nullptr, hold_levels);
}

// SPEC §6.19: the multi-stage form plus the report of a frame with a reference mask
int nct_seq_frame_ref_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_multi_levels* levels,
                                    const nct_color_stages* const* color, const nct_seq_levels* seq_levels, const nct_seq_hold_levels* hold_levels,
                                    const nct_ref_region_levels* region_levels, const nct_seq_pull_levels* pull_levels) {
    return seq_frame_run(ctx, src_bgr, out_bgr, timing, levels, color, false, seq_levels, nullptr, hold_levels, region_levels, pull_levels);
}

int nct_seq_frame(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing) {
    return nct_seq_frame_levels(ctx, src_bgr, out_bgr, timing, nullptr, nullptr);
}

// SPEC §6.5: what a propagated frame enqueues — the frame's pyramid, per level L_t and (motion on) the field, the warp of the kept X' and the packed map, then the
// finish of the last level run on the kept X' and the frame's own pixels, and the download. Nothing upstream of the finish runs. L_t goes straight into the state:
// on this path nothing reads L_(t-1) but the search, which reads its packed form
// With a region mask (SPEC §6.13 rule 3) all of that runs unchanged on the unmixed state; then the last level run's X'_t is mixed with that level's mask into scratch of
// the call, the finish reads the mixed map and composes. Only the level masks down to that level are built. rlv (nullable): where the mixed map and those masks go
// With a reference mask (SPEC §6.19) the kept pull P' of every level run is carried like the labels; the top level run's P' takes P_l's place in SPEC §6.12 rules 4-5: the
// mix mask is min(P', the source's level mask), the compose mask P' at the size the finish targets, then the minimum with the source mask there — kept as fin_mask for
// nct_pair_fit_lut. plv (nullable): where the carried maps go
static int propagate_run(nct_ctx* ctx, pair_state* P, seq_state* q, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* slv, const nct_ref_region_levels* rlv,
                         const nct_seq_pull_levels* plv) {
    const hipStream_t s = ctx->stream;
    const bool ref_masked = P->ref_masked();
    P->fin_mask.reset();
    const nct_params& prm = q->prm;
    const int H = P->sh, W = P->sw, top = prm.levels - 1;
    const size_t N = (size_t)H * W;
    MARK(NCT_ST_OTHER, 0);
    DevBuf<uint8_t> s_lab_full(ctx, N * 3), out_lab(ctx, N * 3), spyr[4];
    if (!s_lab_full.ok() || !out_lab.ok()) return NCT_ERR_HIP;
    NCT_TRY(nctk_bgr2lab(ctx, s, P->src, s_lab_full, N));
    const uint8_t* simg[5]; simg[4] = P->src;
    for (int l = 3; l >= 0; --l) NCT_TRY(pyramid_level(ctx, s, spyr[l], simg, q->ah, q->aw, l));
    MARK(NCT_ST_OTHER, 0);
    if (q->motion && !q->warp_x.reserve(ctx, 6 * (size_t)q->ah[top] * q->aw[top])) return NCT_ERR_HIP;
    if (!P->out.reserve(ctx, N * 3)) return NCT_ERR_HIP;
    for (int l = 0; l <= top; ++l) {
        const int h = q->ah[l], w = q->aw[l];
        const size_t n = (size_t)h * w;
        NCT_TRY(nctk_bgr2lab(ctx, s, simg[l], q->keep_lab[l], n));
        if (q->motion) {
            NCT_TRY(seq_motion_level(ctx, s, q, l, q->keep_lab[l]));
            NCT_TRY(nctk_seq_warp(ctx, s, q->keep_x[l], h, w, q->field[l], q->warp_x));
            // the scratch has the last level's size: there the two maps change places, elsewhere the warped map is copied back
            if (l == top) q->keep_x[l].swap(q->warp_x);
            else NCT_HIP(hipMemcpyAsync(q->keep_x[l], q->warp_x, sizeof(double) * 6 * n, hipMemcpyDeviceToDevice, s));
            NCT_TRY(nctk_seq_pack(ctx, s, q->keep_lab[l], (int)n, q->keep_pk[l]));
            if (q->keep_label[l]) {
                // several references (SPEC §6.18 rule 7): the kept labels follow the field too, out of place through scratch of the call
                DevBuf<uint8_t> carried(ctx, n);
                if (!carried.ok()) return NCT_ERR_HIP;
                NCT_TRY(nctk_label_carry(ctx, s, q->keep_label[l], h, w, q->field[l], carried));
                NCT_HIP(hipMemcpyAsync(q->keep_label[l], carried, n, hipMemcpyDeviceToDevice, s));
            }
            if (ref_masked) {
                // SPEC §6.19: the kept pull follows the field as well — the same byte gather, into the sequence's second map; the two change places
                NCT_TRY(nctk_label_carry(ctx, s, q->keep_pull[l], h, w, q->field[l], q->pull_alt[l]));
                q->keep_pull[l].swap(q->pull_alt[l]);
            }
            // SPEC §6.23 rule 5: the kept fields of every reference follow the field too, so that they always refer to the newest frame
            if (q->carry && q->carry_kept) for (int k = 0; k < P->K; ++k) NCT_TRY(seq_carry_move(ctx, s, q, l, k));
        }
        if (ref_masked && plv) NCT_TRY(dbg_copy(ctx, s, plv->p_held[l], q->keep_pull[l], n));
        if (slv) {
            if (slv->ab_blend[l]) NCT_HIP(hipMemcpyAsync(slv->ab_blend[l], q->keep_x[l], sizeof(double) * 6 * n, hipMemcpyDeviceToHost, s));
            if (slv->motion[l]) {
                if (q->motion) NCT_HIP(hipMemcpyAsync(slv->motion[l], q->field[l], sizeof(int16_t) * 2 * n, hipMemcpyDeviceToHost, s));
                else memset(slv->motion[l], 0, sizeof(int16_t) * 2 * n);
            }
            if (slv->tau_map[l]) std::fill(slv->tau_map[l], slv->tau_map[l] + n, 1.0);          // the previous frame's weight
        }
    }
    if (P->mask && q->tracking) {
        // SPEC §6.14: the level loop has left the frame's fields in place; the matte follows the last level run's (and, SPEC §6.15, is snapped to the frame) before the level masks are built. Its time is other_ms
        MARK(NCT_ST_COLOR, top);
        NCT_TRY(seq_track_step(ctx, s, P, q, nullptr, s_lab_full));
        MARK(NCT_ST_OTHER, 0);
    } else NCT_TRY(seq_track_step(ctx, s, P, q, nullptr, s_lab_full));      // only marks a new matte used
    // the kept (warped) X' of the last level run finishes on the frame's own pixels: at the working size, or (SPEC §6.9 rule 3) on the original frame
    ctx->tm_level = top;
    int wls_it[6] = {0, 0, 0, 0, 0, 0};
    const nct_color_debug dbg{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wls_it};
    full_lab fl;
    NCT_TRY(fl.open(ctx, s, q->target()));
    const int h = q->ah[top], w = q->aw[top];
    const nct_color_debug* const d = timing ? &dbg : nullptr;
    if (P->mask || ref_masked) {
        // only the source's level masks down to the last level run are built; m_top, the F scratch and the mixed map are scratch of this call, requested by the step
        DevBuf<uint8_t> mpyr[4], m_top, f_work; DevBuf<double> x_mix;
        const uint8_t* mimg[5] = {};
        mimg[4] = P->mask;
        if (P->mask) NCT_TRY(source_mask_levels(ctx, s, mpyr, mimg, q->ah, q->aw, top));
        masked_fin mf{ref_masked ? (const uint8_t*)q->keep_pull[top] : nullptr, mimg[top], P->mask, P->src, P->protect, true, nullptr};
        NCT_TRY(finish_level_masked(ctx, s, mf, q->keep_x[top], x_mix, m_top, f_work, P->fin_mask, h, w, H, W, s_lab_full, out_lab, P->out, q->target(), fl, nct_color_params_of(prm), d,
                                    nct_cube_form(prm)));
        // the report: the last level run only; with a source mask alone also the level masks that were built
        if (rlv) {
            const size_t n = (size_t)h * w;
            if (ref_masked) NCT_TRY(dbg_copy(ctx, s, rlv->mask_full[top], mf.f_l, (size_t)mf.fh * mf.fw));
            NCT_TRY(dbg_copy(ctx, s, rlv->ab_mix[top], (double*)x_mix, 6 * n));
            if (ref_masked) NCT_TRY(dbg_copy(ctx, s, rlv->mask[top], mf.m_l, n));
            else for (int l = top; l < 5; ++l) NCT_TRY(dbg_copy(ctx, s, rlv->mask[l], mimg[l], (size_t)q->ah[l] * q->aw[l]));
        }
    } else NCT_TRY(finish_level(ctx, s, q->keep_x[top], h, w, H, W, s_lab_full, out_lab, P->out, q->target(), fl, nct_color_params_of(prm), d, nct_cube_form(prm)));
    if (timing) timing->wls_iters[top] = *std::max_element(wls_it, wls_it + 6);
    MARK(NCT_ST_COLOR, top);
    if (q->target()) NCT_D2H(out_bgr, P->full_out, (size_t)q->full.H * q->full.W * 3);
    else NCT_D2H(out_bgr, P->out, N * 3);
    NCT_SYNC();
    return NCT_OK;
}

int nct_seq_frame_propagate_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels) {
    return nct_seq_frame_propagate_region_levels(ctx, src_bgr, out_bgr, timing, seq_levels, nullptr);
}

// the body of the propagated forms. region_levels: a source mask's report (SPEC §6.13); ref_region_levels, pull_levels: a reference mask's (SPEC §6.19); all nullable
static int seq_propagate_form(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels, const nct_region_levels* region_levels,
                              const nct_ref_region_levels* ref_region_levels, const nct_seq_pull_levels* pull_levels) {
    NCT_CTX_ENTER();
    NCT_OPEN_SEQ(P, "seq_frame_propagate");
    seq_state* q = P->seq;
    if (q->frames == 0) return ctx->fail(NCT_ERR_STATE, "seq_frame_propagate: the sequence has no state to propagate (the first frame after nct_seq_begin / nct_seq_reset is nct_seq_frame's)");
    NCT_REQUIRE(src_bgr && out_bgr, "seq_frame_propagate: null image");
    if (region_levels && !P->mask) return ctx->fail(NCT_ERR_STATE, "seq_frame_propagate: region levels asked for, but no region mask is set (nct_seq_set_region first)");
    if ((ref_region_levels || pull_levels) && !P->ref_masked())
        return ctx->fail(NCT_ERR_STATE, "seq_frame_propagate: reference region levels asked for, but no reference mask is set (nct_seq_set_ref_region first)");
    // SPEC §6.19: a reference mask whose pull no full frame has kept yet (before the first one, or since a set, replace or remove) has nothing to carry
    if (P->ref_masked() && !q->pull_kept)
        return ctx->fail(NCT_ERR_STATE, "seq_frame_propagate: a reference mask is set but no full frame has pulled it yet: a full frame (nct_seq_frame) must come first");
    nct_ref_region_levels qlv;
    if (region_levels) { qlv = ref_region_levels_of(*region_levels); ref_region_levels = &qlv; }
    run_clock clock(ctx, timing, q->prm.flags);
    int rc = seq_upload_frame(ctx, P, q, src_bgr);
    if (rc == NCT_OK) rc = propagate_run(ctx, P, q, out_bgr, timing, seq_levels, ref_region_levels, pull_levels);
    if (rc == NCT_OK) P->finished = true;                        // nct_seq_set_region cleared it: this frame is the result of the new settings
    clock.stop();
    // a frame that failed may have replaced the state of some levels only: the next frame starts over
    if (rc) { (void)hipStreamSynchronize(ctx->stream); q->frames = 0; q->gap = 0; q->acc = 0; q->carry_kept = false; return rc; }
    q->frames += 1; q->gap += 1;
    return clock.read(false);
}

int nct_seq_frame_propagate_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels,
                                          const nct_region_levels* region_levels) {
    return seq_propagate_form(ctx, src_bgr, out_bgr, timing, seq_levels, region_levels, nullptr, nullptr);
}

int nct_seq_frame_propagate_ref_region_levels(nct_ctx* ctx, const uint8_t* src_bgr, uint8_t* out_bgr, nct_pair_timing* timing, const nct_seq_levels* seq_levels,
                                              const nct_ref_region_levels* region_levels, const nct_seq_pull_levels* pull_levels) {
    return seq_propagate_form(ctx, src_bgr, out_bgr, timing, seq_levels, nullptr, region_levels, pull_levels);
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
    if (q->target()) NCT_TRY(upload_shrunk(ctx, src_bgr, q->full.H, q->full.W, frame, P->sh, P->sw));     // SPEC §6.9: the original frame into scratch of its own size
    else NCT_H2D(frame, src_bgr, N * 3);
    const uint8_t* simg[5]; simg[4] = frame;
    for (int l = 3; l >= 0; --l) NCT_TRY(pyramid_level(ctx, s, spyr[l], simg, q->ah, q->aw, l));
    NCT_TRY(seq_field_chain(ctx, s, q, simg, lambda, lab));
    NCT_TRY(nctk_seq_change(ctx, s, lab[lambda], q->keep_lab[lambda], q->ah[lambda], q->aw[lambda], q->motion ? q->field[lambda] : nullptr, threshold, d_rec));
    NCT_D2H(rec, d_rec, sizeof *rec);
    NCT_SYNC();
    return NCT_OK;
}

// the checks of nct_seq_probe / nct_seq_frame_auto, then the probe and the decision; first_ok: a sequence without state is NCT_SEQ_FIRST, not an error
static int seq_probe_decide(nct_ctx* ctx, const char* who, const uint8_t* src_bgr, const nct_seq_auto* a, bool first_ok, nct_seq_auto* used, nct_seq_decision* d) {
    NCT_OPEN_SEQ(P, who);
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
    // SPEC §6.19: a reference mask whose pull no full frame has kept yet has nothing to carry — the one place where a decision depends on a mask
    if (d.kind == NCT_SEQ_PROPAGATED && ((pair_state*)ctx->pair)->ref_masked() && !q->pull_kept) d.kind = NCT_SEQ_KEY;
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

}  // extern "C"

int seq_set_region_dev(nct_ctx* ctx, const uint8_t* d_mask, const nct_region_params* region) { return seq_set_region_from(ctx, d_mask, region, hipMemcpyDeviceToDevice); }
