// The console driver's options: the reference's command-line parser re-created, what a run was asked to do (Config), and the rules that refuse a combination.
#pragma once
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "nct.h"

constexpr int MAX_SIZE = 1000;                 // Config.h:5
struct Param { std::string flag, comment; enum { STR, INT, DBL } kind; void* dst; bool listed = true; };   // listed: the help prints it
// Utility::CmdLine (CmdLine.h:58-69,132-147; CmdLine.cpp:21-56,93-109) re-created; pinned against the reference's own parser compiled unmodified
// (oracle/ref_cmdline.cpp -> tests/golden/cmdline_ref.json -> tests/test_cli.py). The rules, all the reference's:
//  * a token is an "argument" when it starts with '-' or '/' (Parameter::IsArg) — "-5" and "/x" included; any other token is a positional file (collected, unused);
//  * "-h" "-?" "-help" (and the '/' forms) print the help and end the run; an argument that names no parameter prints "Unrecognized parameter: …", the help, and ends it;
//  * the token after a parameter is its value unless it is missing, empty or itself an argument (TParm::Parse) — then the parameter keeps its value and the
//    token is looked at again; numbers are read with operator>> (so "12abc" is 12, "abc" is 0, "3.7" for -g is 3).
// Two portable extensions, each a case the reference ends with "Unrecognized parameter" (recorded as such in the fixture): a value of the form -<digit|.>… is taken
// as a negative number by numeric parameters, and a value that starts with '/' but names no parameter is taken as a unix path by the string parameters (the reference
// is a Windows tool: "-m /data/models" cannot be passed to it at all). A string value keeps its blanks (operator>> into a std::string stops at the first one).
struct CmdLine {
    std::vector<Param> params;
    int files = 0;
    void add(const char* flag, std::string& v, const char* c) { params.push_back({flag, c, Param::STR, &v}); }
    void add(const char* flag, int& v, const char* c) { params.push_back({flag, c, Param::INT, &v}); }
    void add(const char* flag, double& v, const char* c) { params.push_back({flag, c, Param::DBL, &v}); }
    // parsed like every other parameter, but not printed by the help: the help's text is recorded byte for byte (tests/golden/cli_messages.json) and stays what it
    // was; such parameters are described in README.md and SPEC.md
    void unlisted() { params.back().listed = false; }
    static bool is_arg(const char* a) { return a && (a[0] == '-' || a[0] == '/'); }                       // Parameter::IsArg, CmdLine.h:68-70
    static bool is_help(const std::string& a) { return a == "h" || a == "?" || a == "help"; }              // CmdLine.cpp:93-100
    bool names_a_parameter(const char* a) const {
        const std::string n(a + 1);
        if (is_help(n)) return true;
        for (const auto& p : params) if (n == p.flag) return true;
        return false;
    }
    bool is_value(const Param& p, const char* v) const {                                                    // TParm::Parse's test, CmdLine.h:133-136, + the two extensions
        if (!v || !*v) return false;
        if (!is_arg(v)) return true;
        if (p.kind != Param::STR) return v[0] == '-' && ((v[1] >= '0' && v[1] <= '9') || v[1] == '.');
        return v[0] == '/' && !names_a_parameter(v);
    }
    void help(const char* prog) const {
        std::cout << "Running: " << prog << std::endl;
        for (const auto& p : params) {                                          // TParm::Print, CmdLine.h:140-142
            if (!p.listed) continue;
            std::cout << "-" << p.flag << ": " << "(default=";
            if (p.kind == Param::STR) std::cout << *(const std::string*)p.dst;
            else if (p.kind == Param::INT) std::cout << *(const int*)p.dst;
            else std::cout << *(const double*)p.dst;
            std::cout << ") " << p.comment << std::endl;
        }
    }
    bool parse(int argc, char** argv, int first = 1) {
        int i = first;
        while (i < argc) {
            if (!is_arg(argv[i])) { ++files; ++i; continue; }              // positional "files" are collected and never used (CmdLine.cpp:26-29)
            const std::string a(argv[i] + 1);
            if (is_help(a)) { help(argv[0]); return false; }
            bool done = false;
            for (const auto& p : params)
                if (a == p.flag) {
                    if (i + 1 < argc && is_value(p, argv[i + 1])) {
                        if (p.kind == Param::STR) *(std::string*)p.dst = argv[i + 1];
                        else { std::istringstream is(argv[i + 1]); if (p.kind == Param::INT) is >> *(int*)p.dst; else is >> *(double*)p.dst; }
                        ++i;
                    }
                    ++i; done = true; break;
                }
            if (!done) { std::cout << "Unrecognized parameter: " << argv[i] << std::endl << std::endl; help(argv[0]); return false; }
        }
        return true;
    }
};

// What the run was asked to do. The option table binds its flags to these members, which therefore keep the types the help prints their defaults in
struct Config {
    std::string input_dir, output_dir, model_dir;      // -i, -o, -m
    nct_params prm;                                    // -bds, -eps, -nl, -l, -w as parsed; seed, levels and flags once settle() has run (main sets the library's defaults in all the nct_ blocks)
    int gpu = 0, ngpus = 1;                            // -g, -gpus: the first device and how many
    int inflight = 1, io = -1, pin = 1;                // -inflight: contexts per GPU; -io: threads of the decode / encode pool (-1: two per GPU); -pin: NUMA pinning
    int seed = 1, levels = 5, feat16 = 0;              // -seed, -levels (clamped to [1, 5]), -feat16 1: fp16 PatchMatch features
    int resume = 0, vis = 0;                           // -resume 1: skip lines whose outputs are complete; -vis 1: the per-level dumps
    int procs = 0, world = 1, rank = 0, steal = 0, rccl = 0;   // -procs N forks N ranks; -world / -rank: this process's place; -steal 1: shared ticket counter; -rccl 1
    int fullres = 0;                                   // -fullres 1 / 2: the content image's own size with the exact or the upsampling finish (SPEC §6.1 / §6.8)
    int seq = 0, seqfull = 0; nct_seq_params sp;       // -seq 1, -tau, -sigma: sequences (SPEC §6.3); -seqfull 1 / 2: at full resolution, exact or upsampling finish (SPEC §6.9)
    int upguide = 0; nct_guided_params gp;             // -upguide 1, -upsigma: the guided modifier of the upsampling finish (SPEC §6.10), set on every context
    int motion = 0; nct_seq_motion mp;                 // -motion 1, -mr0, -mr, -mpen: motion-compensated blend (SPEC §6.4)
    int key = 1;                                       // -key N: every N-th frame of a sequence is a full one (SPEC §6.5)
    int carry = 0, carryiters = -1;                    // -carry 1, -carryiters n: correspondence carry (SPEC §6.23); -1 (only where -carryiters is not given): the sequence's own iterations
    int autokey = 0; nct_seq_auto ap;                  // -autokey 1, -keythr, -keycut, -keychange, -keygap: key frames chosen per frame (SPEC §6.7)
    int lut = 0, lutfull = 0; double lut_lambda = 0.0; // -lut N (0 = off), -lutfull 1, -lutlambda (0 = the library's default) (SPEC §6.6)
    std::string mask_dir, refmask_dir; int maskprotect = 0;   // -mask / -refmask <dir>: region masks by content / reference file name (SPEC §6.11 / §6.12), -maskprotect 0 / 1
    std::string reflib_dir; int refk = 1, reftap = 5, refcenter = 1;   // -reflib <dir>, -refk K, -reftap t, -refcenter 0 / 1: a line whose reference is "auto" takes the K best of the library (SPEC §6.21)
    int grid = 0; double grid_lambda = 0.0;            // -grid G (0 = off): nodes along the longer side of a local colour grid, -gridlambda (0 = the library's default) (SPEC §6.22)
};
void add_options(CmdLine& cl, Config& cfg);            // the option table, in the help's order
// the first rule the parsed options break, as the text behind "Error: " (empty: accepted). lutlambda_given, gridlambda_given, carryiters_given: "-lutlambda" / "-gridlambda" / "-carryiters" was on the
// command line
std::string option_refusal(const Config& cfg, bool lutlambda_given, bool gridlambda_given = false, bool carryiters_given = false);
// after the checks (and -procs' fork, which changes -gpus): seed, levels and flags into prm, the clamps of -gpus, -inflight and -io
void settle(Config& cfg);
