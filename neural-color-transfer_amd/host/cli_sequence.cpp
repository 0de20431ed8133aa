#include "cli_job.h"
#include "jpeg_io.h"

std::vector<Group> plan_groups(const std::vector<Pair>& pairs) {
    std::vector<Group> g;
    long nseq = 0;
    for (size_t i = 0; i < pairs.size(); ++i) {
        const Pair& p = pairs[i];
        const bool frame = p.err.empty() && p.refs.size() == 1;
        if (frame && !g.empty() && g.back().seq >= 0 && pairs[g.back().first].stl == p.stl && pairs[g.back().first].bds == p.bds) { ++g.back().count; continue; }
        g.push_back({i, 1, frame ? nseq++ : -1});
    }
    return g;
}

// one sequence on one context, its frames in file order. The reference is decoded and shrunk once; a frame whose (shrunk) size differs from the open sequence's begins
// a new one at that frame (-seqfull: nothing is shrunk here, the library takes and returns originals, and it is the frame's ORIGINAL size that counts); a line that cannot be decoded is skipped and the state continues from the last good frame; with -resume 1 the sequence is skipped only if
// every output is complete, else it is redone from its first frame. With -key N the k-th frame run since the last nct_seq_begin is a full frame iff k % N == 0 and a
// propagated one (SPEC §6.5) otherwise; a frame that failed left the sequence reset, so the next one is full. With -autokey 1 every frame goes through
// nct_seq_frame_auto (SPEC §6.7) and the log says what each frame after a sequence's first turned out to be. Returns the number of lines it finished
size_t run_sequence(nct_ctx* ctx, const Config& cfg, const std::vector<Pair>& pairs, const Group& g) {
    nct_params prm = cfg.prm;
    prm.bds_weight = pairs[g.first].bds;
    if (cfg.resume) {
        bool all = true;
        for (size_t i = g.first; i < g.first + g.count && all; ++i) all = outputs_complete(cfg, output_name(cfg, pairs[i]));
        if (all) {
            for (size_t i = g.first; i < g.first + g.count; ++i) {
                Job j; j.index = i; j.p = pairs[i]; j.t0 = std::chrono::steady_clock::now(); j.name = output_name(cfg, j.p);
                j.say("Skipping (-resume): %s exists.\n\n", j.name.c_str());
                j.state = Job::SKIPPED; finish(cfg, j);
            }
            return g.count;
        }
    }
    ImageBGR ref; std::string ref_err; bool ref_tried = false, open = false;
    int fh = 0, fw = 0;
    long k = 0;                                                            // frames run since the last nct_seq_begin
    for (size_t i = g.first; i < g.first + g.count; ++i) {
        Job j; j.index = i; j.p = pairs[i];
        load_pair(cfg, j, true);
        if (j.state == Job::LOADED && !ref_tried) {
            ref_tried = true;
            const std::string refStr = cfg.input_dir + "/" + j.p.refs[0];
            if (!imgio::read(refStr, ref, ref_err)) { ref.px.clear(); j.say("Error: Fail reading style image: %s\n", refStr.c_str()); }
            else {
                j.say("Read style file: %s, w = %d, h = %d\n", refStr.c_str(), ref.w, ref.h);
                if (!cfg.seqfull && !shrink(ctx, ref)) { ref_err = nct_last_error(ctx); ref.px.clear(); }
            }
        }
        if (j.state == Job::LOADED && ref.px.empty()) { j.err = "cannot read style image: " + ref_err; j.state = Job::FAILED; }      // logged once, at the frame that tried
        if (j.state == Job::LOADED && (cfg.lutfull || cfg.grid)) j.orig = j.cnt;
        if (j.state == Job::LOADED && !cfg.seqfull && !shrink(ctx, j.cnt)) j.fail(std::string("resize failed: ") + nct_last_error(ctx), nct_last_error(ctx));
        if (j.state == Job::LOADED) {
            int rc = NCT_OK;
            if (!open || j.cnt.h != fh || j.cnt.w != fw) {
                rc = cfg.seqfull ? nct_seq_begin_fullres(ctx, ref.px.data(), ref.h, ref.w, j.cnt.h, j.cnt.w, MAX_SIZE, cfg.seqfull == 2 ? NCT_FINISH_UPSAMPLE : NCT_FINISH_EXACT, &prm, &cfg.sp)
                                 : nct_seq_begin(ctx, ref.px.data(), ref.h, ref.w, j.cnt.h, j.cnt.w, &prm, &cfg.sp);
                open = rc == NCT_OK; fh = j.cnt.h; fw = j.cnt.w; k = 0;
                if (open) j.say("Sequence %ld: begins at this frame (%d x %d, tau = %g, sigma = %g).\n", g.seq, fw, fh, cfg.sp.tau, cfg.sp.sigma);
                if (open && cfg.seqfull) j.say("Sequence %ld: full resolution, %s finish (-seqfull %d).\n", g.seq, cfg.seqfull == 2 ? "upsampling" : "exact", cfg.seqfull);
                if (open && cfg.motion) {
                    rc = nct_seq_set_motion(ctx, &cfg.mp);
                    if (rc == NCT_OK) j.say("Sequence %ld: motion compensation (radius0 = %d, radius = %d, penalty = %d).\n", g.seq, cfg.mp.radius0, cfg.mp.radius, cfg.mp.penalty);
                    else { nct_seq_end(ctx); open = false; }               // no plain sequence where -motion 1 was asked: the next frame begins again
                }
                if (open && cfg.carry) {
                    rc = nct_seq_set_carry(ctx, 1, cfg.carryiters);
                    if (rc == NCT_OK) j.say("Sequence %ld: correspondence carry (%d iterations on frames that merge; -1 = as every frame).\n", g.seq, cfg.carryiters);
                    else { nct_seq_end(ctx); open = false; }               // no plain sequence where -carry 1 was asked: the next frame begins again
                }
            }
            nct_pair_timing tm;
            j.out.resize((size_t)j.cnt.h * j.cnt.w * 3);
            const bool prop = !cfg.autokey && k % cfg.key != 0;
            if (rc == NCT_OK && prop) j.say("Sequence %ld: frame %ld is propagated from the frame before it (-key %d).\n", g.seq, k, cfg.key);
            if (rc == NCT_OK && cfg.autokey) {
                nct_seq_decision d;
                rc = nct_seq_frame_auto(ctx, j.cnt.px.data(), j.out.data(), &tm, &cfg.ap, &d);
                if (rc == NCT_OK && d.kind != NCT_SEQ_FIRST)
                    j.say("Sequence %ld: frame %ld is %s (changed %u of %u at level %d).\n", g.seq, k,
                          d.kind == NCT_SEQ_PROPAGATED ? "propagated" : d.kind == NCT_SEQ_CUT ? "a scene cut" : "a key frame", d.change.changed, d.change.pixels, d.level);
            } else if (rc == NCT_OK) rc = prop ? nct_seq_frame_propagate(ctx, j.cnt.px.data(), j.out.data(), &tm) : nct_seq_frame(ctx, j.cnt.px.data(), j.out.data(), &tm);
            k = rc == NCT_OK ? k + 1 : 0;
            if (rc != NCT_OK) j.fail(nct_last_error(ctx));
            else { job_lut(ctx, cfg, j); log_times(j, prm, tm); store_pair(j); }
        }
        finish(cfg, j);
    }
    if (open) nct_seq_end(ctx);
    return g.count;
}
