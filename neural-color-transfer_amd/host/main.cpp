// neural_color_transfer — the reference's console driver re-created on top of libnct (C ABI, include/nct.h).
// Mirrors: get_input / main (main.cu:29-44, 546-590), transfer_single (main.cu:456-543), Utility::CmdLine
// (CmdLine.h:58-69,132-147; CmdLine.cpp:21-56,93-109). Same flags, same pairs.txt, same output names, same log lines; what differs from the reference, and the
// [extension] flags, are listed in INTEGRATION.md §A. This file: the self-test hooks, option parsing, the -procs fork, model and contexts, NUMA placement, RCCL,
// the threads and the closing lines. The options are in cli_options, one pairs.txt line in cli_job, -vis 1 in cli_vis, -seq 1 in cli_sequence, the threads'
// loops in cli_workers.
#include <sys/stat.h>
#include <sys/wait.h>
#include <algorithm>
#include <cstdlib>
#include <thread>
#include "jpeg_io.h"
#include "affinity.h"
#include "rccl_sync.h"
#include "cli_workers.h"

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--png-roundtrip")) {       // codec self-test hook (no GPU): decode argv[2] (PNG or JPEG), re-encode to argv[3]
        ImageBGR im; std::string err;
        if (!imgio::read(argv[2], im, err)) { printf("Error: %s: %s\n", argv[2], err.c_str()); return 1; }
        if (!pngio::write(argv[3], im.px.data(), im.h, im.w, err)) { printf("Error: %s: %s\n", argv[3], err.c_str()); return 1; }
        printf("%d %d\n", im.w, im.h);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--gpu-locality")) {        // affinity self-test hook (no GPU): NUMA node and CPU list of the PCI device argv[2]
        const affinity::GpuLocality g = affinity::gpu_locality(argv[2]);
        printf("%d %s\n", g.numa_node, affinity::cpus_to_string(g.cpus).c_str());
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "--check-prototxt")) {      // deploy-prototxt self-test hook (no GPU)
        if (nct_vgg19_check_prototxt(nullptr, argv[2]) != NCT_OK) { printf("Error: %s\n", nct_model_last_error()); return 1; }
        printf("ok\n");
        return 0;
    }
    if (nct_version() != NCT_VERSION) { printf("Error: libnct is version %d, this driver was built against %d.\n", nct_version(), NCT_VERSION); return -1; }
    CmdLine cl; Config cfg;
    nct_params_default(&cfg.prm); nct_seq_params_default(&cfg.sp); nct_seq_motion_default(&cfg.mp); nct_seq_auto_default(&cfg.ap); nct_guided_params_default(&cfg.gp);
    add_options(cl, cfg);
    // parser self-test hook (no GPU): `--parse-only <args…>` parses the rest like a normal run and prints what main would go on with, in the format of
    // oracle/ref_cmdline.cpp (the reference's own parser): tests/test_cli.py compares the two on the vectors of tests/golden/cmdline_ref.json
    // job-planning hook (no GPU): `--plan-only <args…>` goes as far as a normal run goes before it creates a context and prints, per pairs.txt line, what it would run
    const bool parse_only = argc >= 2 && !strcmp(argv[1], "--parse-only");
    const bool plan_only = argc >= 2 && !strcmp(argv[1], "--plan-only");
    const bool parsed = cl.parse(argc, argv, parse_only || plan_only ? 2 : 1);
    if (parse_only) {
        std::cout << std::flush;
        printf("@@RESULT rc=%d\n", parsed ? 1 : 0);
        printf("m=%s\ni=%s\no=%s\ng=%d\n", cfg.model_dir.c_str(), cfg.input_dir.c_str(), cfg.output_dir.c_str(), cfg.gpu);
        printf("bds=%.17g\neps=%.17g\nnl=%.17g\nl=%.17g\nw=%.17g\n", cfg.prm.bds_weight, cfg.prm.eps, cfg.prm.nonlocal_weight, cfg.prm.local_weight, cfg.prm.wls_lambda_init);
        printf("files=%d\n", cl.files);
        return 0;
    }
    if (!parsed) return -1;
    const bool lutlambda_given = std::any_of(argv + 1, argv + argc, [](const char* a) { return !strcmp(a, "-lutlambda"); });
    const bool gridlambda_given = std::any_of(argv + 1, argv + argc, [](const char* a) { return !strcmp(a, "-gridlambda"); });
    const bool carryiters_given = std::any_of(argv + 1, argv + argc, [](const char* a) { return !strcmp(a, "-carryiters"); });
    const std::string refused = option_refusal(cfg, lutlambda_given, gridlambda_given, carryiters_given);
    if (!refused.empty()) { printf("Error: %s\n", refused.c_str()); return -1; }
    if (!lutlambda_given) cfg.lut_lambda = 0.0;                             // a value that came in another spelling of the flag does not count
    if (!gridlambda_given) cfg.grid_lambda = 0.0;
    if (!carryiters_given) cfg.carryiters = -1;
    if (!plan_only) mkdir(cfg.output_dir.c_str(), 0777);                    // main.cu:458
    uint64_t run_token = getenv("NCT_RUN_TOKEN") ? strtoull(getenv("NCT_RUN_TOKEN"), nullptr, 0) : 0;      // hand-started ranks of one run share it (and remove <output>/.rccl_id between runs)
    const std::string tickets_path = cfg.output_dir + "/.tickets";
    if (cfg.procs > 0 && !plan_only) {
        // one process per GPU: fork BEFORE anything touches the HIP runtime (a forked HIP context is unusable), every child goes on as rank r of `procs` on device -g + r
        if (cfg.world != 1) { printf("Error: -procs and -world are exclusive (-procs sets -world for its children).\n"); return -1; }
        if (cfg.steal) { unlink(tickets_path.c_str()); }                     // a fresh counter for this run
        run_token = ((uint64_t)getpid() << 32) ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();      // children are forks: they inherit it; an id file of another run carries another token
        fflush(stdout);
        std::vector<pid_t> kids;
        int my = -1;
        for (int r = 0; r < cfg.procs; ++r) {
            const pid_t k = fork();
            if (k < 0) { printf("Error: fork failed.\n"); return -1; }
            if (k == 0) { my = r; break; }
            kids.push_back(k);
        }
        if (my < 0) {                                                       // the parent only waits: exit status = the worst child's
            const auto t0 = std::chrono::steady_clock::now();
            int worst = 0;
            for (pid_t k : kids) { int st = 0; if (waitpid(k, &st, 0) < 0 || !WIFEXITED(st) || WEXITSTATUS(st) != 0) worst = -1; }
            printf("All %d process(es) finished in %.3f sec%s.\n", cfg.procs, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), worst ? " (at least one failed)" : "");
            return worst;
        }
        cfg.world = cfg.procs; cfg.rank = my; cfg.gpu += my; cfg.ngpus = 1;
    }
    settle(cfg);
    const int ngpus = cfg.ngpus, nworkers = cfg.ngpus * cfg.inflight;
    const std::string pairsFile = cfg.input_dir + "/pairs.txt";
    FILE* fp = fopen(pairsFile.c_str(), "r");
    if (!fp) { printf("Error: File %s does not exist in the input directory.\n", pairsFile.c_str()); return -1; }
    std::vector<Pair> pairs;
    char a[260], b[260]; float w = 0.f;
    while (fscanf(fp, "%259s %259s %f\n", a, b, &w) == 3) { pairs.push_back({a, b, w, {}, ""}); split_refs(pairs.back()); }
    fclose(fp);
    const std::vector<Group> groups = cfg.seq ? plan_groups(pairs) : std::vector<Group>();
    RefLibrary reflib;                                                       // -reflib <dir>: listed here, built once the first context has its weights
    if (!cfg.reflib_dir.empty()) {
        const std::string why = list_reference_library(cfg, reflib);
        if (!why.empty()) { printf("Error: %s\n", why.c_str()); return -1; }
    }
    if (plan_only) {
        std::vector<std::string> seq_of(pairs.size());               // -seq 1: " seq=<sequence>:<index>" behind the lines that are frames, -key N: " prop" behind the propagated ones; -autokey 1: " auto" behind every frame but a sequence's first (what it becomes is known only when it runs)
        for (const Group& g : groups)
            if (g.seq >= 0) for (size_t i = 0; i < g.count; ++i)
                seq_of[g.first + i] = " seq=" + std::to_string(g.seq) + ":" + std::to_string(i) + (cfg.autokey ? (i ? " auto" : "") : (i % (size_t)cfg.key ? " prop" : ""));
        for (size_t i = 0; i < pairs.size(); ++i) {
            const Pair& p = pairs[i];
            const std::string why = refusal(cfg, p);
            if (!why.empty()) { printf("@@JOB error=%s\n", why.c_str()); continue; }
            std::string refs;
            for (size_t k = 0; k < p.refs.size(); ++k) refs += (k ? "|" : "") + p.refs[k];
            printf("@@JOB src=%s refs=%s bds=%.6g out=%s%s\n", p.cnt.c_str(), refs.c_str(), (double)p.bds, output_name(cfg, p).c_str(), seq_of[i].c_str());
        }
        return 0;
    }

    // model: <model_dir>/vgg19/VGG_ILSVRC_19_layers_deploy.prototxt + VGG_ILSVRC_19_layers.caffemodel (main.cu:575-580; '\\' or '/' accepted in model_dir).
    // The topology is built into the library, so the prototxt is only checked: a directory that describes another network is refused, a missing file is noted.
    const std::string proto = cfg.model_dir + "/vgg19/VGG_ILSVRC_19_layers_deploy.prototxt", model = cfg.model_dir + "/vgg19/VGG_ILSVRC_19_layers.caffemodel";
    struct stat pst;
    if (stat(proto.c_str(), &pst) == 0) {
        if (nct_vgg19_check_prototxt(nullptr, proto.c_str()) != NCT_OK) { printf("Error: %s\n", nct_model_last_error()); return -1; }
    } else printf("Note: %s not found; using the library's built-in VGG19 topology (conv1_1 ... relu5_1).\n", proto.c_str());

    // test hook: NCT_DEVICE_OVERRIDE=d runs every logical GPU of -gpus N on HIP device d (the N > 1 host path on a 1-GPU box)
    const char* ovr = getenv("NCT_DEVICE_OVERRIDE");
    auto device_of = [&](int g) { return ovr && *ovr ? atoi(ovr) : cfg.gpu + g; };
    // one context (streams, arena) per worker; worker j runs on GPU j mod G, so -inflight K gives every GPU K independent pairs whose
    // launch-latency-bound phases (coarse pyramid levels, solver reductions) overlap with the other pairs' heavy kernels.
    // Weights: the 575 MB caffemodel is parsed ONCE per process, uploaded ONCE per device, and every other context of that device shares the read-only copy
    // (the reference parses it twice, main.cu:581-582; round 2 of this CLI parsed and uploaded it once per worker).
    std::vector<nct_ctx*> ctxs(nworkers, nullptr);
    nct_model* host_model = nullptr;
    if (nct_model_parse_caffemodel(model.c_str(), &host_model) != NCT_OK) { printf("Error: %s\n", nct_model_last_error()); return -1; }
    int uploads = 0;
    for (int j = 0; j < nworkers; ++j) {
        const int g = j % ngpus, dev = device_of(g);
        if (nct_create(dev, &ctxs[j]) != NCT_OK) { printf("Error: %s\n", nct_last_error(nullptr)); return -1; }
        if (j < ngpus) { char name[256]; nct_device_name(ctxs[j], name, sizeof name); printf("Set device %d: %s.\n", dev, name); }
        if (cfg.upguide && nct_set_finish_guided(ctxs[j], &cfg.gp) != NCT_OK) { printf("Error: %s\n", nct_last_error(ctxs[j])); return -1; }
        int owner = -1;
        for (int k = 0; k < j; ++k) if (device_of(k % ngpus) == dev) { owner = k; break; }
        const int rc = owner < 0 ? (++uploads, nct_vgg19_load_model(ctxs[j], host_model)) : nct_vgg19_share_weights(ctxs[j], ctxs[owner]);
        if (rc != NCT_OK) { printf("Error: %s\n", nct_last_error(ctxs[j])); return -1; }
    }
    nct_model_free(host_model);
    { size_t wb = 0; nct_vgg19_weights_info(ctxs[0], nullptr, &wb, nullptr);
      printf("VGG19 weights: parsed once, %d device cop%s of %.1f MB shared by %d context(s).\n", uploads, uploads == 1 ? "y" : "ies", wb / 1e6, nworkers); }
    if (!cfg.reflib_dir.empty()) {                                           // once per process; the workers share it read-only, each context keeps its own device copy of the rows
        const std::string why = build_reference_library(ctxs[0], cfg, reflib);
        if (!why.empty()) { printf("Error: %s\n", why.c_str()); return -1; }
    }

    // NUMA placement: the CPUs next to each GPU (sysfs), for its workers and its share of the I/O pool
    std::vector<affinity::GpuLocality> loc(ngpus);
    if (cfg.pin)
        for (int g = 0; g < ngpus; ++g) {
            char addr[32];
            if (nct_device_pci_bus_id(device_of(g), addr, sizeof addr) != NCT_OK) continue;
            loc[g] = affinity::gpu_locality(addr);
            if (!loc[g].cpus.empty()) printf("GPU %d (%s): NUMA node %d, host threads pinned to CPUs %s.\n", device_of(g), addr, loc[g].numa_node, affinity::cpus_to_string(loc[g].cpus).c_str());
        }

    // -rccl 1: one communicator over the ranks of this run (one process per GPU), used for the start barrier and for the two reductions at the end — never on a pair's data path
    rccl_sync::Group rg;
    const std::string rccl_id_path = cfg.output_dir + "/.rccl_id";
    if (cfg.rccl) {
        if (ngpus != 1) printf("Note: -rccl 1 is for one process per GPU (-procs / -world); this process drives %d GPUs and joins with its first.\n", ngpus);
        if (!rg.init(cfg.world, cfg.rank, device_of(0), rccl_id_path, run_token) || !rg.barrier())
            printf("Note: -rccl 1: no RCCL group (%s); rank %d goes on without the barrier.\n", rg.why().c_str(), cfg.rank);
        else printf("RCCL: rank %d of %d joined, start barrier passed.\n", cfg.rank, cfg.world);
    }
    const auto t0 = std::chrono::steady_clock::now();
    // pairs are independent and of mixed sizes: every worker takes the next decoded pair (work stealing inside the node, BASELINE config 5);
    // which worker runs a pair has no influence on its result
    std::vector<std::thread> threads;
    Pipeline P; P.cap = (size_t)std::max(2, 2 * nworkers);
    P.tickets.total = cfg.seq ? groups.size() : pairs.size(); P.tickets.rank = cfg.rank; P.tickets.world = cfg.world;
    if (cfg.world > 1 && cfg.steal) {
        P.tickets.fd = open(tickets_path.c_str(), O_RDWR | O_CREAT, 0644);     // 8 bytes: the next line to hand out (absent or short = 0). A hand-started set of ranks removes it between runs.
        if (P.tickets.fd < 0) { printf("Error: cannot open %s for -steal.\n", tickets_path.c_str()); return -1; }
    }
    if (const char* e = getenv("NCT_IO_READY_MB")) P.byte_cap = (size_t)std::max(0L, atol(e)) << 20;      // test hook: decoded backlog allowed in front of the GPU workers (default 1 GiB)
    const int io = cfg.seq ? 0 : cfg.io;                                     // -seq 1: every worker does its own file I/O
    auto pinned = [&](int k) { if (cfg.pin) affinity::pin_current_thread(loc[k % ngpus].cpus); };
    for (int t = 0; t < io; ++t) threads.emplace_back([&, t] { pinned(t); io_thread(P, cfg, pairs); });
    for (int j = 0; j < nworkers; ++j)
        threads.emplace_back([&, j] { pinned(j); if (io > 0) gpu_worker(P, ctxs[j], cfg); else self_serving_worker(P, ctxs[j], cfg, pairs, groups); });
    for (auto& t : threads) t.join();
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const size_t done = P.taken;
    if (P.tickets.fd >= 0) close(P.tickets.fd);
    if (cfg.world > 1) printf("Rank %d of %d: ", cfg.rank, cfg.world);
    printf("Processed %zu pair(s) on %d GPU(s), %d in flight each, %d I/O thread(s), in %.3f sec (%.3f pairs/sec).\n", done, ngpus, cfg.inflight, io, sec, done == 0 ? 0.0 : done / sec);
    if (rg.ok()) {
        double sec_max = sec, total = (double)done;
        const bool r1 = rg.reduce(sec, rccl_sync::kMax, &sec_max), r2 = rg.reduce((double)done, rccl_sync::kSum, &total);
        if (r1 && r2) { if (cfg.rank == 0) printf("All %d rank(s) over RCCL: %.0f pair(s) in %.3f sec = MAX over ranks (%.3f pairs/sec).\n", cfg.world, total, sec_max, sec_max > 0 ? total / sec_max : 0.0); }
        else printf("Note: RCCL reduction failed (%s).\n", rg.why().c_str());
        rg.finish(rccl_id_path);
    }
    for (auto* c : ctxs) nct_destroy(c);
    nct_reflib_free(reflib.lib);
    return 0;
}
