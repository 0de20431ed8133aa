#include "cli_job.h"
#include <dirent.h>
#include <algorithm>
#include <mutex>
#include "cube_io.h"
#include "jpeg_io.h"

namespace {
std::mutex g_print, g_status;
const RefLibrary* g_library = nullptr;                // -reflib: set by build_reference_library before the workers start, read-only afterwards

std::string stem(const std::string& path) {          // main.cu:524-531 (find_last_of on both separators, strip the extension)
    const size_t pos = path.find_last_of("\\/") + 1;
    const size_t dot = path.find_last_of('.');
    return path.substr(pos, dot == std::string::npos || dot < pos ? std::string::npos : dot - pos);
}
std::string json_escape(const std::string& s) {
    std::string o;
    for (char c : s) { if (c == '"' || c == '\\') { o += '\\'; o += c; } else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; } else o += c; }
    return o;
}
// one JSON line per pair in <output_dir>/status.jsonl (batch bookkeeping for -resume; absent in the reference)
void write_status(const Config& cfg, const Job& j) {
    const bool skipped = j.state == Job::SKIPPED;
    // one process per GPU (-world N): every rank appends to its own file, status.<rank>.jsonl — appends of different processes to one file could interleave
    FILE* f = fopen((cfg.output_dir + (cfg.world > 1 ? "/status." + std::to_string(cfg.rank) + ".jsonl" : std::string("/status.jsonl"))).c_str(), "a");
    if (!f) return;
    fprintf(f, "{\"pair\": %zu, \"content\": \"%s\", \"style\": \"%s\", \"bds\": %.6g, \"status\": \"%s\", \"output\": \"%s\", \"seconds\": %.4f, \"message\": \"%s\"}\n",
            j.index, json_escape(j.p.cnt).c_str(), json_escape(j.p.stl).c_str(), j.p.bds, j.state == Job::DONE ? "done" : (skipped ? "skipped" : "error"), json_escape(j.name).c_str(),
            skipped ? 0.0 : j.secs(), json_escape(skipped ? "output exists" : j.err).c_str());
    fclose(f);
}
// what a job writes beside <name>.png: <name>.cube with -lut N, <name>_lut.png with -lutfull 1
std::string cube_name(const std::string& png) { return png.substr(0, png.size() - 4) + ".cube"; }
std::string lutfull_name(const std::string& png) { return png.substr(0, png.size() - 4) + "_lut.png"; }
std::string grid_name(const std::string& png) { return png.substr(0, png.size() - 4) + "_grid.png"; }      // -grid G
// -mask / -refmask <dir>: the image in/x.png uses <dir>/x.png (or .jpg) where it exists; the mask has the image's size as decoded and is its file's first channel.
// flag, whose, what: the words by which the two kinds' messages differ. mask stays empty where there is no file; false: the job has failed
bool load_mask(Job& j, const std::string& dir, const std::string& image_path, const ImageBGR& img, const char* flag, const char* whose, const char* what, std::vector<uint8_t>& mask) {
    for (const char* ext : {".png", ".jpg"}) {
        const std::string mpath = dir + "/" + stem(image_path) + ext;
        FILE* f = fopen(mpath.c_str(), "rb");
        if (!f) continue;
        fclose(f);
        ImageBGR m; std::string err;
        if (!imgio::read(mpath, m, err)) { j.fail("Fail reading mask image: " + mpath, "cannot read mask image: " + err); return false; }
        if (m.h != img.h || m.w != img.w) {
            char why[400]; snprintf(why, sizeof why, "%s: %s is %d x %d, the %s image %d x %d", flag, mpath.c_str(), m.w, m.h, whose, img.w, img.h);
            j.fail(why); return false;
        }
        mask.resize((size_t)m.h * m.w);
        for (size_t i = 0; i < mask.size(); ++i) mask[i] = m.px[3 * i + 2];      // BGR in memory: the file's first channel is R
        j.say("Read %s file: %s\n", what, mpath.c_str());
        break;
    }
    return true;
}
}  // namespace

void finish(const Config& cfg, Job& j) {           // status line + the pair's log block, printed in one piece
    { std::lock_guard<std::mutex> g(g_status); write_status(cfg, j); }
    std::lock_guard<std::mutex> g(g_print); fputs(j.log.c_str(), stdout); fflush(stdout);
}

// shrink so that the longer side is <= MAX_SIZE, int truncation as in main.cu:500-522
bool shrink(nct_ctx* ctx, ImageBGR& img) {
    if (img.w <= MAX_SIZE && img.h <= MAX_SIZE) return true;
    int cw = MAX_SIZE, ch = (int)(cw / (float)img.w * img.h);
    if (img.w < img.h) { ch = MAX_SIZE; cw = (int)(ch / (float)img.h * img.w); }
    ImageBGR out; out.h = ch; out.w = cw; out.px.resize((size_t)ch * cw * 3);
    if (nct_resize_u8c3(ctx, img.px.data(), img.h, img.w, out.px.data(), ch, cw) != NCT_OK) return false;
    img = std::move(out);
    return true;
}

// the second token of a pairs.txt line: one name, or several separated by commas (SPEC §6.2). More than NCT_MAX_REFS names or an empty one refuse the line
void split_refs(Pair& p) {
    p.refs.clear(); p.err.clear();
    if (p.stl.find(',') == std::string::npos) { p.refs.push_back(p.stl); return; }
    size_t pos = 0;
    for (;;) {
        const size_t c = p.stl.find(',', pos);
        p.refs.push_back(p.stl.substr(pos, c == std::string::npos ? std::string::npos : c - pos));
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    for (const auto& r : p.refs) if (r.empty()) { p.err = "empty reference name in \"" + p.stl + "\""; return; }
    if (p.refs.size() > (size_t)NCT_MAX_REFS) p.err = std::to_string(p.refs.size()) + " references in one line, at most " + std::to_string(NCT_MAX_REFS) + " are supported";
}
// the line's own fault, or an option it cannot be combined with
std::string refusal(const Config& cfg, const Pair& p) {
    if (!p.err.empty()) return p.err;
    if (is_auto(p) && cfg.reflib_dir.empty()) return "the reference \"auto\" needs -reflib <dir>";
    if (cfg.fullres && p.refs.size() > 1) return cfg.fullres == 2 ? "-fullres 2 cannot be combined with several references" : "-fullres 1 cannot be combined with several references";
    return "";
}
// <out>/<src stem>_<ref stem>_<bds %2.2f>.png (main.cu:524-537); with several references their stems joined by '+'
std::string output_name(const Config& cfg, const Pair& p) {
    std::string refs;
    for (size_t k = 0; k < p.refs.size(); ++k) refs += (k ? "+" : "") + stem(cfg.input_dir + "/" + p.refs[k]);
    char name[2048];
    snprintf(name, sizeof name, "%s/%s_%s_%2.2f.png", cfg.output_dir.c_str(), stem(cfg.input_dir + "/" + p.cnt).c_str(), refs.c_str(), (double)p.bds);
    return name;
}
// -resume: every file of the job's output is there and complete
bool outputs_complete(const Config& cfg, const std::string& png) {
    return pngio::looks_complete(png) && (!cfg.lut || cubeio::looks_complete(cube_name(png), cfg.lut)) && (!cfg.lutfull || pngio::looks_complete(lutfull_name(png))) &&
           (!cfg.grid || pngio::looks_complete(grid_name(png)));
}

// -grid G: the local colour grid of a finished job (SPEC §6.22), fitted from the equal-sized source and result the job holds and applied to the content image at its
// original size. G nodes along the longer side, the shorter side in proportion, 16 along luma. A grid that cannot be made does not take the result with it
static void job_grid(nct_ctx* ctx, const Config& cfg, Job& j) {
    nct_grid_params gp; nct_grid_params_default(&gp);
    const int h = j.cnt.h, w = j.cnt.w, lng = std::max(h, w), sht = std::min(h, w);
    const int other = std::max(2, (int)((2LL * cfg.grid * sht + lng) / (2LL * lng)));      // round(G * short / long), halves up
    gp.gy = h >= w ? cfg.grid : other; gp.gx = h >= w ? other : cfg.grid; gp.gz = 16;
    if (cfg.grid_lambda > 0.0) gp.lambda = cfg.grid_lambda;
    std::vector<double> grid((size_t)gp.gy * gp.gx * gp.gz * 12);
    int rc = nct_grid_fit(ctx, j.cnt.px.data(), j.out.data(), h, w, &gp, grid.data(), nullptr);
    if (rc == NCT_OK) {
        j.grid_out.resize(j.orig.px.size());
        rc = nct_grid_apply(ctx, grid.data(), gp.gy, gp.gx, gp.gz, j.orig.px.data(), j.orig.h, j.orig.w, j.grid_out.data());
    }
    if (rc != NCT_OK) { j.grid_err = nct_last_error(ctx); j.grid_out.clear(); return; }
    j.say("Local colour grid: %d x %d x %d, lambda = %g.\n", gp.gy, gp.gx, gp.gz, gp.lambda);
}

// -lut N: the table of a finished job (SPEC §6.6), fitted through the host-pointer call from the equal-sized source and result the job holds; -lutfull 1: that table
// on the content image at its original size. Before log_times, which drops the inputs. With -grid G the job's grid comes first, from the same images
void job_lut(nct_ctx* ctx, const Config& cfg, Job& j) {
    if (cfg.grid) job_grid(ctx, cfg, j);
    if (cfg.grid && !cfg.lutfull) { j.orig.px.clear(); j.orig.px.shrink_to_fit(); }
    if (!cfg.lut) return;
    nct_lut_params lp; nct_lut_params_default(&lp);
    lp.size = cfg.lut;
    if (cfg.lut_lambda > 0.0) lp.lambda = cfg.lut_lambda;
    j.lut.resize((size_t)lp.size * lp.size * lp.size * 3);
    // a masked line's table is fitted over its region (SPEC §6.11 rule 7); without a mask this is nct_lut_fit
    // a line with a reference mask: over the last level's target mask, which the context that has just run the line still holds (SPEC §6.12 rule 7)
    int rc = j.ref_masked() ? nct_pair_fit_lut(ctx, &lp, j.lut.data())
                            : nct_lut_fit_masked(ctx, j.cnt.px.data(), j.out.data(), j.mask.empty() ? nullptr : j.mask.data(), (size_t)j.cnt.h * j.cnt.w, &lp, j.lut.data(), nullptr);
    if (rc == NCT_OK && cfg.lutfull) {
        j.lut_out.resize(j.orig.px.size());
        rc = nct_lut_apply(ctx, j.lut.data(), lp.size, j.orig.px.data(), (size_t)j.orig.h * j.orig.w, j.lut_out.data());
        j.orig.px.clear(); j.orig.px.shrink_to_fit();
    }
    // a table that cannot be made (a full-resolution source above the fit's 2^26 pixels, for one) does not take the computed result with it: store_pair writes the
    // image, then reports the job as failed for its table
    if (rc != NCT_OK) { j.lut_err = nct_last_error(ctx); j.lut.clear(); j.lut_out.clear(); return; }
    j.lut_n = lp.size;
    j.say("Look-up table: %d x %d x %d, lambda = %g.\n", lp.size, lp.size, lp.size, lp.lambda);
}

// the line's reference images, names under `dir`, and with -refmask their masks; false: the job has failed
static bool load_refs(const Config& cfg, Job& j, const std::string& dir) {
    std::string err;
    j.refs.resize(j.p.refs.size());
    for (size_t k = 0; k < j.refs.size(); ++k) {
        const std::string refStr = dir + "/" + j.p.refs[k];
        if (!imgio::read(refStr, j.refs[k], err)) { j.fail("Fail reading style image: " + refStr, "cannot read style image: " + err); return false; }
        j.say("Read style file: %s, w = %d, h = %d\n", refStr.c_str(), j.refs[k].w, j.refs[k].h);
    }
    if (cfg.refmask_dir.empty()) return true;
    j.refmask.resize(j.refs.size());
    for (size_t k = 0; k < j.refs.size(); ++k)
        if (!load_mask(j, cfg.refmask_dir, dir + "/" + j.p.refs[k], j.refs[k], "-refmask", "style", "reference mask", j.refmask[k])) return false;
    return true;
}

// in_seq: the line is a frame of a sequence (-seq 1) — its resume check and its reference belong to the sequence, not to the line
void load_pair(const Config& cfg, Job& j, bool in_seq) {
    j.t0 = std::chrono::steady_clock::now();
    j.log += "-----------------***********************----------------------\n";
    j.say("Content: %s, style: %s, BDS weight: %f.\n", j.p.cnt.c_str(), j.p.stl.c_str(), (double)j.p.bds);
    const std::string why = refusal(cfg, j.p);
    if (!why.empty()) { j.fail(why); return; }
    const std::string cntStr = cfg.input_dir + "/" + j.p.cnt;
    j.name = output_name(cfg, j.p);                                         // a line with "auto": until its references are chosen
    if (!in_seq && !is_auto(j.p) && cfg.resume && outputs_complete(cfg, j.name)) {           // a truncated file (killed run, full disk) is redone, not skipped
        j.say("Skipping (-resume): %s exists.\n\n", j.name.c_str());
        j.state = Job::SKIPPED; return;
    }
    std::string err;
    if (!imgio::read(cntStr, j.cnt, err)) { j.fail("Fail reading content image: " + cntStr, "cannot read content image: " + err); return; }
    j.say("\n**Read content file: %s, w = %d, h = %d\n", cntStr.c_str(), j.cnt.w, j.cnt.h);
    if (in_seq) return;
    if (!cfg.mask_dir.empty() && !load_mask(j, cfg.mask_dir, cntStr, j.cnt, "-mask", "content", "mask", j.mask)) return;
    if (is_auto(j.p)) return;                                               // its references are chosen on the GPU worker: choose_references
    load_refs(cfg, j, cfg.input_dir);
}

// the reference's per-level lines (main.cu:331; ColorTransfer.cpp:1373,1434), then its total (main.cu:453); the decoded inputs are dropped
void log_times(Job& j, const nct_params& prm, const nct_pair_timing& tm) {
    for (int l = 0; l < prm.levels; ++l) {
        j.say("Patch Match Time: %lf sec.\n", (tm.pm_level_ms[l] + tm.vote_level_ms[l]) * 1e-3);
        j.say("Nonlocal Solve Time: %lf\n", tm.nonlocal_level_ms[l] * 1e-3);
        j.say("WLS Solve Time: %lf\n", tm.wls_level_ms[l] * 1e-3);
    }
    j.say("VGG19 Time: %lf sec.\n", tm.vgg_ms * 1e-3);
    j.say("**Finished Time: %lf sec.\n", tm.total_ms * 1e-3);
    j.refs.clear(); j.refs.shrink_to_fit();
    j.cnt.px.clear(); j.cnt.px.shrink_to_fit();                 // the store stage needs only cnt.h / cnt.w
}
// -reflib (SPEC §6.21): the library's images in byte order of their names
std::string list_reference_library(const Config& cfg, RefLibrary& L) {
    L.dir = cfg.reflib_dir;
    DIR* d = opendir(L.dir.c_str());
    if (!d) return "-reflib: cannot open the directory " + L.dir + ".";
    while (const dirent* e = readdir(d)) {
        const std::string n(e->d_name);
        const size_t dot = n.find_last_of('.');
        std::string ext = dot == std::string::npos || dot == 0 ? "" : n.substr(dot);
        std::transform(ext.begin(), ext.end(), ext.begin(), [](unsigned char c) { return (char)tolower(c); });
        if (ext == ".png" || ext == ".jpg" || ext == ".jpeg") L.names.push_back(n);
    }
    closedir(d);
    std::sort(L.names.begin(), L.names.end());                  // std::string orders by unsigned bytes
    if (L.names.empty()) return "-reflib: " + L.dir + " holds no image (.png, .jpg).";
    if (L.names.size() > 4096) return "-reflib: " + L.dir + " holds " + std::to_string(L.names.size()) + " images, a library holds at most 4096.";
    return "";
}

// pass 1 (with -refcenter 1): every image's tap through nct_vgg19_features, its channel sums accumulated in double, image after image, in raster order — the centre
// is their mean as fp32. Pass 2: nct_reflib_add per image
std::string build_reference_library(nct_ctx* ctx, const Config& cfg, RefLibrary& L) {
    static const int tapC[5] = {64, 128, 256, 512, 512};
    const int tap = cfg.reftap, C = tapC[tap - 1];
    std::vector<ImageBGR> imgs(L.names.size());
    std::string err;
    for (size_t k = 0; k < imgs.size(); ++k) {
        const std::string path = L.dir + "/" + L.names[k];
        if (!imgio::read(path, imgs[k], err)) return "-reflib: cannot read " + path + ": " + err;
        if (!shrink(ctx, imgs[k])) return "-reflib: " + path + ": " + nct_last_error(ctx);
    }
    std::vector<float> center;
    if (cfg.refcenter) {
        std::vector<double> acc((size_t)C, 0.0);
        double cells = 0.0;
        std::vector<float> F;
        for (size_t k = 0; k < imgs.size(); ++k) {
            const int ht = ((imgs[k].h - 1) >> (tap - 1)) + 1, wt = ((imgs[k].w - 1) >> (tap - 1)) + 1;
            const size_t n = (size_t)ht * wt;
            F.resize(n * C);
            float* taps[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            taps[tap - 1] = F.data();
            if (nct_vgg19_features(ctx, imgs[k].px.data(), imgs[k].h, imgs[k].w, 3 * imgs[k].w, tap, taps, nullptr) != NCT_OK)
                return "-reflib: " + L.dir + "/" + L.names[k] + ": " + nct_last_error(ctx);
            for (int c = 0; c < C; ++c) for (size_t i = 0; i < n; ++i) acc[c] += (double)F[(size_t)c * n + i];
            cells += (double)n;
        }
        center.resize((size_t)C);
        for (int c = 0; c < C; ++c) center[c] = (float)(acc[c] / cells);
    }
    if (nct_reflib_create(tap, C, cfg.refcenter ? center.data() : nullptr, &L.lib) != NCT_OK) return std::string("-reflib: ") + nct_last_error(nullptr);
    for (size_t k = 0; k < imgs.size(); ++k)
        if (nct_reflib_add(ctx, L.lib, imgs[k].px.data(), imgs[k].h, imgs[k].w) != NCT_OK) return "-reflib: " + L.dir + "/" + L.names[k] + ": " + nct_last_error(ctx);
    printf("Reference library: %zu image(s) of %s at tap %d, %s.\n", L.names.size(), L.dir.c_str(), tap, cfg.refcenter ? "centred on their mean tap vector" : "not centred");
    g_library = &L;
    return "";
}

// a line with "auto": its content image, shrunk as the run will shrink it, is ranked against the library; the first -refk entries become the line's references
static bool choose_references(nct_ctx* ctx, const Config& cfg, Job& j) {
    const RefLibrary& L = *g_library;
    ImageBGR work = j.cnt;
    if (!shrink(ctx, work)) { j.fail(std::string("resize failed: ") + nct_last_error(ctx), nct_last_error(ctx)); return false; }
    const size_t N = L.names.size(), K = std::min((size_t)cfg.refk, N);
    std::vector<int32_t> order(N); std::vector<int64_t> key(N);
    if (nct_reflib_rank(ctx, L.lib, work.px.data(), work.h, work.w, nullptr, order.data(), key.data(), nullptr, nullptr) != NCT_OK) { j.fail(nct_last_error(ctx)); return false; }
    j.p.refs.clear(); j.p.stl.clear();
    std::string chosen;
    for (size_t k = 0; k < K; ++k) {
        j.p.refs.push_back(L.names[order[k]]);
        j.p.stl += (k ? "," : "") + L.names[order[k]];
        chosen += (k ? ", " : "") + L.names[order[k]] + " (key " + std::to_string((long long)key[order[k]]) + ")";
    }
    j.say("Reference library: chose %s of %zu.\n", chosen.c_str(), N);
    j.name = output_name(cfg, j.p);
    return load_refs(cfg, j, L.dir);
}

void run_pair(nct_ctx* ctx, const Config& cfg, Job& j) {
    if (is_auto(j.p) && !choose_references(ctx, cfg, j)) return;
    nct_params prm = cfg.prm;
    prm.bds_weight = j.p.bds;                                   // the per-line weight overrides -bds (main.cu:475)
    nct_pair_timing tm;                                         // stage times come from stream events: asking for them adds no host synchronisation
    nct_region_params region; nct_region_params_default(&region); region.protect = cfg.maskprotect;
    const uint8_t* mask = j.mask.empty() ? nullptr : j.mask.data();   // -mask: the line runs masked (SPEC §6.11); null: every call below is the unmasked one
    if (cfg.fullres) {                                          // -fullres 1 / 2: the library shrinks both images itself and returns the content image at its own size
        const ImageBGR& stl = j.refs[0];
        j.out.resize((size_t)j.cnt.h * j.cnt.w * 3);
        // a reference mask (SPEC §6.12) goes in at the reference's original size and takes the exact finish: -fullres 2 with -refmask was refused at the start
        const int rc = (!j.refmask.empty() && !j.refmask[0].empty()) ? nct_process_pair_fullres_ref_region(ctx, j.cnt.px.data(), j.cnt.h, j.cnt.w, mask, stl.px.data(), stl.h, stl.w, j.refmask[0].data(), MAX_SIZE,
                                                                            &region, &prm, j.out.data(), &tm)
                                      : nct_process_pair_fullres_finish_region(ctx, j.cnt.px.data(), j.cnt.h, j.cnt.w, mask, stl.px.data(), stl.h, stl.w, MAX_SIZE, cfg.fullres == 2 ? NCT_FINISH_UPSAMPLE : NCT_FINISH_EXACT, &region, &prm,
                                                              j.out.data(), &tm);
        if (rc != NCT_OK) j.fail(nct_last_error(ctx));
        else { job_lut(ctx, cfg, j); log_times(j, prm, tm); }
        return;
    }
    if (cfg.lutfull || cfg.grid) j.orig = j.cnt;
    const int cnt_h = j.cnt.h, cnt_w = j.cnt.w;                 // as decoded: the mask's size until it is shrunk too
    bool shrunk = shrink(ctx, j.cnt);
    // a mask shrinks with its image, by the same routine on the replicated three-channel image (= the single-channel resize, SPEC §6.11 rule 1)
    auto shrink_mask = [&](std::vector<uint8_t>& mk, int oh, int ow) {
        ImageBGR m; m.h = oh; m.w = ow; m.px.resize(mk.size() * 3);
        for (size_t i = 0; i < mk.size(); ++i) m.px[3 * i] = m.px[3 * i + 1] = m.px[3 * i + 2] = mk[i];
        if (!shrink(ctx, m)) return false;
        mk.resize((size_t)m.h * m.w);
        for (size_t i = 0; i < mk.size(); ++i) mk[i] = m.px[3 * i];
        return true;
    };
    for (size_t k = 0; k < j.refs.size(); ++k) {
        const int oh = j.refs[k].h, ow = j.refs[k].w;
        shrunk = shrunk && shrink(ctx, j.refs[k]);
        if (shrunk && k < j.refmask.size() && !j.refmask[k].empty() && (oh != j.refs[k].h || ow != j.refs[k].w)) shrunk = shrink_mask(j.refmask[k], oh, ow);
    }
    if (mask && j.mask.size() != (size_t)j.cnt.h * j.cnt.w) {
        shrunk = shrunk && shrink_mask(j.mask, cnt_h, cnt_w);
        if (shrunk) mask = j.mask.data();
    }
    if (!shrunk) { j.fail(std::string("resize failed: ") + nct_last_error(ctx), nct_last_error(ctx)); return; }
    j.out.resize((size_t)j.cnt.h * j.cnt.w * 3);
    // what the library takes of the references; one of them runs as a pair, several as SPEC §6.2's list — under the entry points whose names the error texts carry
    const int K = (int)j.refs.size();
    std::vector<const uint8_t*> px(K); std::vector<int> rh(K), rw(K);
    for (int k = 0; k < K; ++k) { px[k] = j.refs[k].px.data(); rh[k] = j.refs[k].h; rw[k] = j.refs[k].w; }
    std::string err; bool ok;
    std::vector<const uint8_t*> qs(K, nullptr);                 // -refmask: the references' masks (SPEC §6.12); null: that reference has none
    for (int k = 0; k < K && k < (int)j.refmask.size(); ++k) if (!j.refmask[k].empty()) qs[k] = j.refmask[k].data();
    const uint8_t* const* refmasks = j.ref_masked() ? qs.data() : nullptr;
    if (cfg.vis) {
        std::string pre(j.name); pre.resize(pre.size() - 4);    // the output file's stem
        ok = run_with_vis({ctx, j.cnt, K, px.data(), rh.data(), rw.data(), prm, pre, j.out.data(), &tm, err, mask, &region, refmasks});
    } else {
        // NULL masks are the plain forms (nct.h): one call per kind of upload, whatever -mask and -refmask gave
        ok = (K > 1 ? nct_process_multi_ref_region(ctx, j.cnt.px.data(), j.cnt.h, j.cnt.w, mask, K, px.data(), rh.data(), rw.data(), refmasks, &region, &prm, j.out.data(), &tm)
                    : nct_process_pair_ref_region(ctx, j.cnt.px.data(), j.cnt.h, j.cnt.w, mask, px[0], rh[0], rw[0], qs[0], &region, &prm, j.out.data(), &tm)) == NCT_OK;
        if (!ok) err = nct_last_error(ctx);
    }
    if (!ok) { j.fail(err); return; }
    job_lut(ctx, cfg, j);
    log_times(j, prm, tm);
}
void store_pair(Job& j) {
    std::string err;
    if (!pngio::write(j.name, j.out.data(), j.cnt.h, j.cnt.w, err)) { j.fail("cannot write " + j.name + ": " + err, "cannot write output: " + err); return; }
    if (!j.lut.empty()) {
        if (!cubeio::write(cube_name(j.name), j.lut.data(), j.lut_n, err)) { j.fail(err, "cannot write table: " + err); return; }
        j.say("Look-up table file: %s.\n", cube_name(j.name).c_str());
    }
    if (!j.lut_out.empty()) {
        if (!pngio::write(lutfull_name(j.name), j.lut_out.data(), j.orig.h, j.orig.w, err)) { j.fail("cannot write " + lutfull_name(j.name) + ": " + err, "cannot write output: " + err); return; }
        j.say("Look-up table on the original: %s.\n", lutfull_name(j.name).c_str());
    }
    if (!j.grid_out.empty()) {
        if (!pngio::write(grid_name(j.name), j.grid_out.data(), j.orig.h, j.orig.w, err)) { j.fail("cannot write " + grid_name(j.name) + ": " + err, "cannot write output: " + err); return; }
        j.say("Local colour grid on the original: %s.\n", grid_name(j.name).c_str());
    }
    j.say("Final output file: %s.\n\n", j.name.c_str());
    if (!j.lut_err.empty()) { j.fail("no look-up table: " + j.lut_err); return; }
    if (!j.grid_err.empty()) { j.fail("no local colour grid: " + j.grid_err); return; }
    j.state = Job::DONE;
}
void run_line(nct_ctx* ctx, const Config& cfg, const Pair& p, size_t index) {
    Job job; job.index = index; job.p = p;
    load_pair(cfg, job);
    if (job.state == Job::LOADED) run_pair(ctx, cfg, job);
    if (job.state == Job::LOADED) store_pair(job);
    finish(cfg, job);
}
