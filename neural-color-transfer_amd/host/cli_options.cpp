#include "cli_options.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <thread>

void add_options(CmdLine& cl, Config& cfg) {
    cl.add("m", cfg.model_dir, "Directory of network models.");
    cl.add("i", cfg.input_dir, "Input directory of content and style images and pairs.txt.");
    cl.add("o", cfg.output_dir, "Output directory of result images.");
    // the reference's comment strings (main.cu:32-43); its "(default: ...)" remarks quote other numbers than Config::Config() sets
    // (Config.h:58-72) — the leading "(default=...)" that CmdLine prints (CmdLine.h:140-142) is the value that really applies
    cl.add("g", cfg.gpu, "GPU ID (default: 0).");
    cl.add("bds", cfg.prm.bds_weight, "Weight of reverse color in BDS voting (default: 2.0).");
    cl.add("eps", cfg.prm.eps, "Eps is used to avoid dividing zero (default: 0.6 with range in [0-255]).");
    cl.add("nl", cfg.prm.nonlocal_weight, "Weight of nonlocal constraint (default: 0.4.");
    cl.add("l", cfg.prm.local_weight, "Weight of local constraitn (default: 0.001).");
    cl.add("w", cfg.prm.wls_lambda_init, "Initial value of WLS weight (default: 0.0234375).");
    cl.add("gpus", cfg.ngpus, "[extension] number of GPUs to shard pairs.txt over, starting at -g (default: 1).");
    cl.add("inflight", cfg.inflight, "[extension] pairs in flight per GPU, one context + host thread each (default: 1; 2-4 raises throughput ~20 %).");
    cl.add("io", cfg.io, "[extension] threads of the shared decode/encode pool (default -1: two per GPU, at most the machine's; 0: every GPU worker does its own file I/O).");
    cl.add("pin", cfg.pin, "[extension] 1 = pin each GPU's worker and I/O threads to the CPUs of the GPU's NUMA node (sysfs local_cpulist); 0 = leave the scheduler alone.");
    cl.add("seed", cfg.seed, "[extension] seed of the counter-based RNG (default: 1).");
    cl.add("levels", cfg.levels, "[extension] pyramid levels to run, coarse to fine: 5 = the full L=5..1 loop, 1 = L=5 only.");
    cl.add("resume", cfg.resume, "[extension] 1 = skip pairs whose output file exists and is a complete PNG; every pair appends a JSON line to <output>/status.jsonl.");
    cl.add("vis", cfg.vis, "[extension] 1 = the reference's ENABLE_VIS dumps per level (flow maps, level images, error heat map, coefficient and cluster images) next to the output.");
    cl.add("fullres", cfg.fullres, "[extension] 1 = return the content image at its own size: the pyramid runs at most 1000 px on a side, its last level's WLS finish at the original size (SPEC 6.1); 2 = the same with the upsampling finish: that finish stays at the working size and its smoothed coefficient maps are upsampled onto the original pixels (SPEC 6.8); not with -vis 1.");
    cl.add("procs", cfg.procs, "[extension] N > 0: fork N processes, one per GPU (-g, -g + 1, ...): process r runs with -rank r -world N on its own device, HIP runtime and status.<r>.jsonl (the process-per-GPU shape; -gpus N keeps all GPUs in one process).");
    cl.add("world", cfg.world, "[extension] number of cooperating processes that share this pairs.txt and output directory (default 1); set by -procs, or by hand with -rank.");
    cl.add("rank", cfg.rank, "[extension] this process's rank in [0, world): it runs the pairs.txt lines i with i mod world = rank (or the ones it draws, -steal 1).");
    cl.add("rccl", cfg.rccl, "[extension] 1 = the ranks of -procs / -world form an RCCL communicator (one rank per GPU, over xGMI on a node): a start barrier, and the job's time = MAX over ranks and its pair count = SUM over ranks by all-reduce, printed by rank 0. Nothing of a pair's data crosses GPUs; without RCCL (or with 0, the default) the ranks simply run.");
    cl.add("steal", cfg.steal, "[extension] 1 = with -world > 1, lines are drawn from a shared counter (<output>/.tickets under a file lock) by whichever rank is free, instead of i mod world: mixed-size batches.");
    cl.add("feat16", cfg.feat16, "[extension] 1 = fp16 PatchMatch feature tiles (fp32 accumulate); not bit-identical to the default (about 45 dB against it).");
    cl.add("seq", cfg.seq, "[extension] 1 = consecutive pairs.txt lines with one and the same reference and weight are the frames of a sequence (SPEC 6.3): one worker runs them in file order and blends each frame's colour coefficients with the previous frame's; every worker does its own file I/O (-io is not used); not with -fullres 1 or -vis 1.");
    cl.add("seqfull", cfg.seqfull, "[extension] -seq 1: 1 = full-resolution sequences (SPEC 6.9): frames are passed and returned at their own size, the sequence's state stays at the working size and the last level's finish runs at the original size; 2 = the same with the upsampling finish (SPEC 6.8); not with -lutfull 1.");
    cl.add("upguide", cfg.upguide, "[extension] -fullres 2 or -seqfull 2: 1 = the upsampling finish is guided by the working-size image (SPEC 6.10): each original pixel weights its 4 x 4 working-size coefficient taps by how well their colour matches its own, which keeps the coefficients' edges sharp.");
    cl.add("upsigma", cfg.gp.sigma, "[extension] -upguide 1: how far a tap's colour may be from the pixel's before its weight halves, in 8-bit Lab units (finite, > 0).");
    cl.add("tau", cfg.sp.tau, "[extension] -seq 1: temporal weight in [0, 1); 0 = every frame on its own.");
    cl.add("sigma", cfg.sp.sigma, "[extension] -seq 1: sensitivity of the blend to changes between frames, in 8-bit Lab units (> 0).");
    cl.add("motion", cfg.motion, "[extension] -seq 1: 1 = motion-compensated blend (SPEC 6.4): every level finds per pixel where it was in the previous frame (5 x 5 block match on the Lab level images, coarse to fine) and blends with the coefficients there.");
    cl.add("mr0", cfg.mp.radius0, "[extension] -motion 1: search radius at the coarsest level, in [0, 8].");
    cl.add("mr", cfg.mp.radius, "[extension] -motion 1: search radius of the refinement at every finer level, in [0, 3].");
    cl.add("mpen", cfg.mp.penalty, "[extension] -motion 1: cost per tap and pixel of displacement from the search centre, in [0, 255].");
    cl.add("key", cfg.key, "[extension] -seq 1: N in [1, 1000]: within a sequence only every N-th frame runs the whole pair; the frames between take their colour coefficients from the frame before them through the motion field and run the last level's finish only (SPEC 6.5). 1 = every frame is a full frame.");
    cl.add("autokey", cfg.autokey, "[extension] -seq 1: 1 = the key frames are chosen per frame (SPEC 6.7): a cheap probe measures how much of the frame the motion field does not explain, and the frame is propagated, runs as a key frame, or restarts the sequence at a scene cut; not with -key N > 1.");
    cl.add("keythr", cfg.ap.threshold, "[extension] -autokey 1: a pixel counts as changed when its three Lab bytes differ from the previous frame's by more than this in sum, in [0, 765].");
    cl.add("keycut", cfg.ap.cut_permille, "[extension] -autokey 1: a frame with at least this many changed pixels per thousand is a scene cut, in [0, 1001]; 1001 = never.");
    cl.add("keychange", cfg.ap.key_permille, "[extension] -autokey 1: a frame is a key frame once the changed pixels since the last full frame reach this many per thousand, in [0, 1001]; 1001 = never.");
    cl.add("keygap", cfg.ap.max_gap, "[extension] -autokey 1: at most this many frames from one full frame to the next, in [1, 1000].");
    cl.add("lut", cfg.lut, "[extension] N in {3, 5, 9, 17, 33, 65}: beside each result image write <same name>.cube, a 3D look-up table of N^3 nodes fitted from the source and the result (SPEC 6.6); works in every mode.");
    cl.add("lutlambda", cfg.lut_lambda, "[extension] -lut N: smoothness weight of the table's fit (> 0; default: the library's, 0.1).");
    cl.add("mask", cfg.mask_dir, "[extension] directory of region masks (SPEC 6.11): a content image in/x.png is recoloured only where <dir>/x.png (or .jpg; its first channel, the content image's size) is not 0 — 255 = the full transfer, between = partial; a line without a mask file runs as without -mask; works with -fullres 1, several references, -lut, -lutfull and -vis 1; not with -fullres 2 or -seq 1.");
    cl.add("refmask", cfg.refmask_dir, "[extension] directory of reference region masks (SPEC 6.12): colours are taken only from where <dir>/y.png (or .jpg; its first channel, the style image's size) of a style image in/y.png is not 0 — 255 = allowed, between = partial; a style image without a mask file counts as allowed everywhere; combines with -mask, -maskprotect, -fullres 1, several references, -lut, -lutfull and -vis 1; not with -fullres 2 or -seq 1.");
    cl.add("maskprotect", cfg.maskprotect, "[extension] -mask / -refmask: 1 = a pixel whose mask is 0 never changes (default 0: the transition follows the image's own edges and may reach such pixels).");
    cl.add("reflib", cfg.reflib_dir, "[extension] directory of graded stills, the reference library (SPEC 6.21): a pairs.txt line whose style field is the word auto ranks its content image against every image of <dir> (.png / .jpg, taken in byte order of their names, shrunk like content images) and runs with the best -refk of them; the output name is that of the same line with those files written out; not with -seq 1; -resume does not skip such a line (its name is known only once it is ranked)."); cl.unlisted();
    cl.add("refk", cfg.refk, "[extension] -reflib: how many of the library's images a line with auto runs with, in [1, 8]; 1 runs as a pair, more as several references."); cl.unlisted();
    cl.add("reftap", cfg.reftap, "[extension] -reflib: the VGG19 tap the images are compared at, 1 (conv1_1) to 5 (conv5_1)."); cl.unlisted();
    cl.add("refcenter", cfg.refcenter, "[extension] -reflib: 1 = the library's mean tap vector is subtracted from every descriptor before it is normalised (wider margins between candidates); 0 = not."); cl.unlisted();
    cl.add("lutfull", cfg.lutfull, "[extension] -lut N: 1 = also write <name>_lut.png, the table applied to the content image at its original size; not with -fullres 1.");
    cl.add("grid", cfg.grid, "[extension] G in [2, 64]: beside each result image write <same name>_grid.png, a local colour grid (SPEC 6.22) of G nodes along the longer side (the shorter side in proportion, 16 along luma) fitted from the source and the result and applied to the content image at its original size; not with -fullres or -seqfull."); cl.unlisted();
    cl.add("carry", cfg.carry, "[extension] -seq 1: 1 = correspondence carry (SPEC 6.23): every full frame after a sequence's first starts each level's PatchMatch from the better of its ordinary start field and the previous frame's match, moved along the motion field."); cl.unlisted();
    cl.add("carryiters", cfg.carryiters, "[extension] -carry 1: PatchMatch iterations of the frames that start from the previous frame's match, in [0, 64] (default: as every other frame)."); cl.unlisted();
    cl.add("gridlambda", cfg.grid_lambda, "[extension] -grid G: ridge weight of the grid's fit, in [1/16, 65536] (default: the library's, 16)."); cl.unlisted();
}

__attribute__((format(printf, 1, 2))) static std::string text(const char* fmt, ...) {
    char t[600]; va_list ap; va_start(ap, fmt); vsnprintf(t, sizeof t, fmt, ap); va_end(ap);
    return t;
}

std::string option_refusal(const Config& c, bool lutlambda_given, bool gridlambda_given, bool carryiters_given) {
    const bool mask = !c.mask_dir.empty(), refmask = !c.refmask_dir.empty();
    auto finite_positive = [](double v) { return v > 0.0 && v <= 1.7976931348623157e308; };
    auto outside = [](int v, int lo, int hi) { return v < lo || v > hi; };
    if (c.world < 1 || c.rank < 0 || c.rank >= c.world) return text("-rank %d is not in [0, -world %d).", c.rank, c.world);
    if (outside(c.fullres, 0, 2)) return text("-fullres %d is not one of 0, 1, 2.", c.fullres);
    if (outside(c.seqfull, 0, 2)) return text("-seqfull %d is not one of 0, 1, 2.", c.seqfull);
    if (c.seqfull && !c.seq) return text("-seqfull %d needs -seq 1 (it chooses how a sequence reaches the frames' own size).", c.seqfull);
    if (outside(c.upguide, 0, 1)) return text("-upguide %d is not one of 0, 1.", c.upguide);
    if (c.upguide && c.fullres != 2 && c.seqfull != 2) return "-upguide 1 needs -fullres 2 or -seq 1 -seqfull 2 (it modifies the upsampling finish).";
    if (!(c.gp.sigma > 0.0 && finite_positive(c.gp.sigma * c.gp.sigma))) return text("-upsigma %g is not finite and greater than 0 (and its square as well).", c.gp.sigma);
    if (c.fullres && c.vis) return text("-fullres %d cannot be combined with -vis 1 (the -vis dumps are working-size images).", c.fullres);
    if (c.seq && c.fullres) return "-seq 1 cannot be combined with -fullres 1 (a sequence runs at the working size only). Full-resolution sequences are -seqfull 1 or 2.";
    if (c.seq && c.vis) return "-seq 1 cannot be combined with -vis 1 (the -vis dumps describe single pairs).";
    if (c.seq && !(c.sp.tau >= 0.0 && c.sp.tau < 1.0)) return text("-tau %g is not in [0, 1).", c.sp.tau);
    if (c.seq && !finite_positive(c.sp.sigma)) return text("-sigma %g is not finite and positive.", c.sp.sigma);
    if (c.motion && !c.seq) return "-motion 1 needs -seq 1 (motion compensation belongs to a sequence's blend).";
    if (c.motion && outside(c.mp.radius0, 0, 8)) return text("-mr0 %d is not in [0, 8].", c.mp.radius0);
    if (c.motion && outside(c.mp.radius, 0, 3)) return text("-mr %d is not in [0, 3].", c.mp.radius);
    if (c.motion && outside(c.mp.penalty, 0, 255)) return text("-mpen %d is not in [0, 255].", c.mp.penalty);
    if (outside(c.carry, 0, 1)) return text("-carry %d is not one of 0, 1.", c.carry);
    if (c.carry && !c.seq) return "-carry 1 needs -seq 1 (the correspondence carry belongs to a sequence).";
    if (carryiters_given && !c.carry) return text("-carryiters %d needs -carry 1.", c.carryiters);
    if (carryiters_given && outside(c.carryiters, 0, 64)) return text("-carryiters %d is not in [0, 64].", c.carryiters);
    if (outside(c.key, 1, 1000)) return text("-key %d is not in [1, 1000].", c.key);
    if (c.key > 1 && !c.seq) return text("-key %d needs -seq 1 (propagated frames belong to a sequence).", c.key);
    if (c.autokey && !c.seq) return "-autokey 1 needs -seq 1 (key frames belong to a sequence).";
    if (c.autokey && c.key > 1) return text("-autokey 1 cannot be combined with -key %d (the key frames are either chosen or on a grid).", c.key);
    if (c.autokey && outside(c.ap.threshold, 0, 765)) return text("-keythr %d is not in [0, 765].", c.ap.threshold);
    if (c.autokey && outside(c.ap.cut_permille, 0, 1001)) return text("-keycut %d is not in [0, 1001].", c.ap.cut_permille);
    if (c.autokey && outside(c.ap.key_permille, 0, 1001)) return text("-keychange %d is not in [0, 1001].", c.ap.key_permille);
    if (c.autokey && outside(c.ap.max_gap, 1, 1000)) return text("-keygap %d is not in [1, 1000].", c.ap.max_gap);
    if (outside(c.maskprotect, 0, 1)) return text("-maskprotect %d is not one of 0, 1.", c.maskprotect);
    if (c.maskprotect && !mask && !refmask) return "-maskprotect 1 needs -mask <dir> or -refmask <dir>.";
    if (refmask && c.fullres == 2) return "-refmask cannot be combined with -fullres 2 (a reference mask with the upsampling finish is not defined, SPEC 6.12); use -fullres 1.";
    if (refmask && c.seq) return "-refmask cannot be combined with -seq 1 (sequences with a reference mask are not defined, SPEC 6.12).";
    if (mask && c.fullres == 2) return "-mask cannot be combined with -fullres 2 (a mask with the upsampling finish is not defined, SPEC 6.11); use -fullres 1.";
    if (mask && c.seq) return "-mask cannot be combined with -seq 1 (sequences with a region mask are not defined, SPEC 6.11).";
    if (outside(c.refk, 1, NCT_MAX_REFS)) return text("-refk %d is not in [1, %d].", c.refk, NCT_MAX_REFS);
    if (outside(c.reftap, 1, 5)) return text("-reftap %d is not in [1, 5].", c.reftap);
    if (outside(c.refcenter, 0, 1)) return text("-refcenter %d is not one of 0, 1.", c.refcenter);
    if (!c.reflib_dir.empty() && c.seq) return "-reflib cannot be combined with -seq 1 (a sequence keeps one reference; rank its first frame on its own and name the result).";
    if (!c.reflib_dir.empty() && c.fullres && c.refk > 1) return text("-refk %d cannot be combined with -fullres %d (several references at full resolution are not defined).", c.refk, c.fullres);
    if (c.lut != 0 && c.lut != 3 && c.lut != 5 && c.lut != 9 && c.lut != 17 && c.lut != 33 && c.lut != 65) return text("-lut %d is not one of 3, 5, 9, 17, 33, 65.", c.lut);
    if (lutlambda_given && !c.lut) return "-lutlambda needs -lut N.";
    if (lutlambda_given && !finite_positive(c.lut_lambda)) return text("-lutlambda %g is not finite and greater than 0.", c.lut_lambda);
    if (c.lutfull && !c.lut) return "-lutfull 1 needs -lut N.";
    if (c.lutfull && c.fullres) return text("-lutfull 1 cannot be combined with -fullres %d (the result already has the original size).", c.fullres);
    if (c.lutfull && c.seqfull) return text("-lutfull 1 cannot be combined with -seqfull %d (the results already have the original size).", c.seqfull);
    if (c.grid != 0 && outside(c.grid, 2, 64)) return text("-grid %d is not in [2, 64].", c.grid);
    if (gridlambda_given && !c.grid) return "-gridlambda needs -grid G.";
    if (gridlambda_given && !(c.grid_lambda >= 1.0 / 16.0 && c.grid_lambda <= 65536.0)) return text("-gridlambda %g is not in [1/16, 65536].", c.grid_lambda);
    if (c.grid && c.fullres) return text("-grid %d cannot be combined with -fullres %d (the result already has the original size).", c.grid, c.fullres);
    if (c.grid && c.seqfull) return text("-grid %d cannot be combined with -seqfull %d (the results already have the original size).", c.grid, c.seqfull);
    return "";
}

void settle(Config& cfg) {
    cfg.prm.seed = (uint32_t)cfg.seed;
    cfg.prm.levels = std::min(std::max(cfg.levels, 1), 5);
    if (cfg.feat16) cfg.prm.flags |= NCT_FLAG_FEAT16;
    if (cfg.inflight <= 1) cfg.prm.flags |= NCT_FLAG_LATENCY;          // one pair at a time per GPU: split WLS solves (same result, -3 ms per 700x700 pair)
    cfg.ngpus = std::max(cfg.ngpus, 1);
    cfg.inflight = std::min(std::max(cfg.inflight, 1), 8);
    const int hw = (int)std::thread::hardware_concurrency();
    if (cfg.io < 0) cfg.io = std::min(2 * cfg.ngpus, hw > 0 ? hw : 2 * cfg.ngpus);
    cfg.io = std::min(cfg.io, 64);
}
