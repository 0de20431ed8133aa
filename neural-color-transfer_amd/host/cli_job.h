// One pairs.txt line as the driver handles it: the line (Pair), its state on the way through load, run and store (Job), and the -seq grouping of lines.
#pragma once
#include <chrono>
#include <cstdio>
#include "png_io.h"
#include "cli_options.h"

// one pairs.txt line. stl is the line's second token as written; refs its names: one, or several where the token holds commas (SPEC §6.2).
// err: why the line is refused (too many or empty names) — reported when its turn comes, the run goes on
struct Pair { std::string cnt, stl; float bds; std::vector<std::string> refs; std::string err; };

// ---- one pair = three stages, so that the GPU workers never wait on zlib (the CLI lost up to 30 % to PNG work):
//   load  (I/O pool)   : resume check, decode both images (PNG / JPEG)
//   run   (GPU worker) : shrink to MAX_SIZE on the GPU, nct_process_pair, the reference's log lines
//   store (I/O pool)   : PNG-encode the result (zlib level 3), status line
// With `-io 0` a GPU worker runs all three itself (the round-2 behaviour).
struct Job {
    size_t index = 0; Pair p; std::string name, log, err;
    ImageBGR cnt; std::vector<uint8_t> out;
    ImageBGR orig;                                               // -lutfull 1, -grid G: the content image as decoded, before the shrink to MAX_SIZE
    std::vector<uint8_t> grid_out; std::string grid_err;        // -grid G: the job's local colour grid on `orig`; why the job has none (its result image is written all the same)
    std::vector<float> lut; std::vector<uint8_t> lut_out;       // -lut N: the job's table; -lutfull 1: the table on `orig`
    std::vector<std::vector<uint8_t>> refmask;                   // -refmask: per reference its region mask, one byte per pixel of refs[k] (empty: that reference has none)
    bool ref_masked() const { for (const auto& q : refmask) if (!q.empty()) return true; return false; }
    std::vector<uint8_t> mask;                                   // -mask: the content image's region mask, one byte per pixel of cnt (empty: the line has none)
    int lut_n = 0; std::string lut_err;                          // the table's size; why the job has no table (its result image is written all the same)
    std::vector<ImageBGR> refs;                                  // the line's references: one, or several (SPEC §6.2)
    size_t input_bytes() const { size_t b = cnt.px.size(); for (const auto& r : refs) b += r.px.size(); return b; }
    std::chrono::steady_clock::time_point t0;
    enum { LOADED, SKIPPED, FAILED, DONE } state = LOADED;
    template <typename... A> void say(const char* fmt, A... a) { char line[1200]; snprintf(line, sizeof line, fmt, a...); log += line; }
    // the job ends here: `logged` goes to the log as an Error line, `status` into the status file
    void fail(const std::string& logged, const std::string& status) { say("Error: %s\n", logged.c_str()); err = status; state = FAILED; }
    void fail(const std::string& text) { fail(text, text); }
    double secs() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
// -reflib <dir> (SPEC §6.21): the run's reference library. names: the image files of <dir> in byte order; lib: their descriptors, entry k = names[k]. Listed and
// built once per process, before the workers start, which then share it read-only: a line whose style field is "auto" ranks its content image against it
struct RefLibrary { std::string dir; std::vector<std::string> names; nct_reflib* lib = nullptr; };
std::string list_reference_library(const Config& cfg, RefLibrary& L);                  // the files (no GPU); the text behind "Error: ", or empty
std::string build_reference_library(nct_ctx* ctx, const Config& cfg, RefLibrary& L);   // the descriptors, on a context with weights; the same. The workers use L from here on
inline bool is_auto(const Pair& p) { return p.refs.size() == 1 && p.refs[0] == "auto"; }
void split_refs(Pair& p);                                        // fills p.refs (and p.err) from p.stl
std::string refusal(const Config& cfg, const Pair& p);           // why this run does not take the line; empty: it runs
std::string output_name(const Config& cfg, const Pair& p);
bool outputs_complete(const Config& cfg, const std::string& png);
bool shrink(nct_ctx* ctx, ImageBGR& img);
void load_pair(const Config& cfg, Job& j, bool in_seq = false);
void run_pair(nct_ctx* ctx, const Config& cfg, Job& j);
void job_lut(nct_ctx* ctx, const Config& cfg, Job& j);
void log_times(Job& j, const nct_params& prm, const nct_pair_timing& tm);
void store_pair(Job& j);
void finish(const Config& cfg, Job& j);
void run_line(nct_ctx* ctx, const Config& cfg, const Pair& p, size_t index);      // load -> run -> store -> finish, all on the calling thread

// -vis 1 (cli_vis.cpp): a line's run with its per-level dumps under <pre>_…; K references px[k] of rh[k] x rw[k]. mask (nullable): the content image's region mask,
// cnt.h x cnt.w (SPEC §6.11). refmasks (nullable): per reference its mask or null (SPEC §6.12)
struct VisLine {
    nct_ctx* ctx; const ImageBGR& cnt; int K; const uint8_t* const* px; const int* rh; const int* rw; const nct_params& prm; const std::string& pre; uint8_t* out;
    nct_pair_timing* tm; std::string& err; const uint8_t* mask; const nct_region_params* region; const uint8_t* const* refmasks;
};
bool run_with_vis(const VisLine& L);

// ---- -seq 1 (SPEC §6.3, cli_sequence.cpp). A group is what one worker context takes in one piece: a sequence — a maximal run of consecutive lines with a single
// reference, the same reference token and the same bds weight — or a single line of any other kind (several references, a refused line), which runs as without -seq
// and ends a run.
struct Group { size_t first = 0, count = 0; long seq = -1; };   // lines [first, first + count); seq: the sequence's number in file order, -1 = not a sequence
std::vector<Group> plan_groups(const std::vector<Pair>& pairs);
size_t run_sequence(nct_ctx* ctx, const Config& cfg, const std::vector<Pair>& pairs, const Group& g);      // returns the number of lines it finished
