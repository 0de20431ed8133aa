// The console driver's pure host pieces under AddressSanitizer + UBSan, without the library: the option parser and the refusal rules on argument vectors, split_refs,
// plan_groups, output_name, and Tickets::draw in its modulo form. Built from host/cli_options.cpp, cli_job.cpp and cli_sequence.cpp with unused sections dropped at
// link time, so nothing of libnct is needed (the parameter blocks start from zeros where the driver starts from the library's defaults: what is checked is memory
// and arithmetic, not text — the text is pinned by tests/golden/cli_messages.json). usage: cli_host_check <file>: one argument vector per line, tokens separated by tabs
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include "cli_workers.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream in(argv[1]);
    std::string line;
    int vectors = 0, parsed = 0, refused = 0;
    while (std::getline(in, line)) {
        std::vector<std::string> tok{"cli_host_check"};
        for (size_t pos = 0;;) { const size_t t = line.find('\t', pos); tok.push_back(line.substr(pos, t == std::string::npos ? t : t - pos)); if (t == std::string::npos) break; pos = t + 1; }
        std::vector<char*> av;
        for (auto& t : tok) av.push_back(&t[0]);
        av.push_back(nullptr);
        Config cfg;
        memset(&cfg.prm, 0, sizeof cfg.prm); memset(&cfg.sp, 0, sizeof cfg.sp); memset(&cfg.mp, 0, sizeof cfg.mp); memset(&cfg.ap, 0, sizeof cfg.ap); memset(&cfg.gp, 0, sizeof cfg.gp);
        CmdLine cl;
        add_options(cl, cfg);
        const bool hook = tok.size() > 1 && (tok[1] == "--plan-only" || tok[1] == "--parse-only");
        ++vectors;
        if (!cl.parse((int)tok.size(), av.data(), hook ? 2 : 1)) continue;
        ++parsed;
        refused += !option_refusal(cfg, line.find("-lutlambda") != std::string::npos).empty();
    }
    CHECK(vectors > 0 && parsed > 0 && refused > 0);

    const std::string nine = "r1,r2,r3,r4,r5,r6,r7,r8,r9", longname(5000, 'x');
    const char* tokens[] = {"", ",", ",,", "a", "a,b", ",a", "a,", "a,,b", "a.png,b.jpg,c", nine.c_str(), longname.c_str()};
    std::vector<Pair> pairs;
    for (const char* t : tokens)
        for (float bds : {2.f, 2.f, 0.5f}) {
            pairs.push_back({"c.png", t, bds, {}, ""});
            Pair& p = pairs.back();
            split_refs(p);
            size_t commas = 0; for (char c : p.stl) commas += c == ',';
            CHECK(p.refs.size() == commas + 1);
            bool empty = false; for (const auto& r : p.refs) empty = empty || r.empty();
            CHECK(p.err.empty() == (commas == 0 || (!empty && p.refs.size() <= (size_t)NCT_MAX_REFS)));
        }
    const std::vector<Group> groups = plan_groups(pairs);
    size_t next = 0; long nseq = 0;
    for (const Group& g : groups) {
        CHECK(g.first == next && g.count >= 1 && (g.seq == -1 || g.seq == nseq));
        CHECK(g.seq >= 0 || g.count == 1);
        for (size_t i = g.first; i < g.first + g.count && g.seq >= 0; ++i) CHECK(pairs[i].refs.size() == 1 && pairs[i].stl == pairs[g.first].stl && pairs[i].bds == pairs[g.first].bds);
        next += g.count; nseq += g.seq >= 0;
    }
    CHECK(next == pairs.size() && plan_groups({}).empty());

    Config cfg;
    for (const char* dir : {"", "in", "a.b/c", "C:\\in\\", longname.c_str()})
        for (const char* name : {"", "x", "x.png", ".png", "d.e/x", "d\\x.tar.gz", longname.c_str()}) {
            cfg.input_dir = dir; cfg.output_dir = dir;
            Pair p{name, std::string(name) + "," + name, 0.25f, {}, ""};
            split_refs(p);
            const std::string out = output_name(cfg, p);
            CHECK(out.size() < 2048 && (out.size() == 2047 || out.substr(out.size() - 9) == "_0.25.png"));
        }

    for (size_t total : {(size_t)0, (size_t)1, (size_t)7, (size_t)64})
        for (int world = 1; world <= 5; ++world) {
            std::vector<int> drawn(total, 0);
            for (int rank = 0; rank < world; ++rank) {
                Tickets t; t.total = total; t.rank = rank; t.world = world;
                long last = -1;
                for (long i; (i = t.draw()) >= 0; last = i) { CHECK(i > last && (size_t)i < total && i % world == rank); ++drawn[(size_t)i]; }
                CHECK(t.draw() == -1);
            }
            for (int d : drawn) CHECK(d == 1);
        }
    printf("vectors %d parsed %d refused %d pairs %zu groups %zu\n", vectors, parsed, refused, pairs.size(), groups.size());
    return 0;
}
