#include "cli_workers.h"
#include <algorithm>

void io_thread(Pipeline& P, const Config& cfg, const std::vector<Pair>& pairs) {
    for (;;) {
        std::unique_ptr<Job> j; bool store = false; size_t idx = 0, reserved = 0;
        {
            std::unique_lock<std::mutex> lk(P.m);
            P.cv.wait(lk, [&] { return !P.results.empty() || P.may_load() || P.all_done(); });
            if (!P.results.empty()) { j = std::move(P.results.front()); P.results.pop_front(); P.results_bytes -= j->out.size(); store = true; }       // encoding first: it frees memory and unblocks workers
            else if (P.may_load()) {
                const long t = P.tickets.draw();
                if (t < 0) { P.exhausted = true; lk.unlock(); P.cv.notify_all(); continue; }
                idx = (size_t)t; ++P.taken; ++P.loading; reserved = P.load_estimate; P.loading_bytes += reserved;
            }
            else return;                                                                                                 // every ticket of this process is finished
        }
        P.cv.notify_all();
        if (store) {
            store_pair(*j); finish(cfg, *j);
            { std::lock_guard<std::mutex> lk(P.m); ++P.finished; }
        } else {
            j.reset(new Job()); j->index = idx; j->p = pairs[idx];
            load_pair(cfg, *j);
            const bool go = j->state == Job::LOADED;
            if (!go) finish(cfg, *j);
            std::lock_guard<std::mutex> lk(P.m);
            --P.loading; P.loading_bytes -= reserved;
            if (go) {
                const size_t b = j->input_bytes();
                P.ready_bytes += b; P.load_estimate = std::max(P.load_estimate, b);
                P.ready.push_back(std::move(j));
            } else ++P.finished;
        }
        P.cv.notify_all();
    }
}

void gpu_worker(Pipeline& P, nct_ctx* ctx, const Config& cfg) {
    for (;;) {
        std::unique_ptr<Job> j;
        {
            std::unique_lock<std::mutex> lk(P.m);
            P.cv.wait(lk, [&] { return !P.ready.empty() || P.loads_done(); });
            if (P.ready.empty()) return;
            j = std::move(P.ready.front()); P.ready.pop_front();
            P.ready_bytes -= j->input_bytes();
        }
        P.cv.notify_all();
        run_pair(ctx, cfg, *j);
        if (j->state == Job::FAILED) {
            finish(cfg, *j);
            { std::lock_guard<std::mutex> lk(P.m); ++P.finished; }
        } else {
            std::unique_lock<std::mutex> lk(P.m);
            P.cv.wait(lk, [&] { return P.results.size() < P.cap; });
            P.results_bytes += j->out.size();
            P.results.push_back(std::move(j));
        }
        P.cv.notify_all();
    }
}

void self_serving_worker(Pipeline& P, nct_ctx* ctx, const Config& cfg, const std::vector<Pair>& pairs, const std::vector<Group>& groups) {
    for (;;) {
        long t; { std::lock_guard<std::mutex> lk(P.m); t = P.tickets.draw(); }
        if (t < 0) return;
        size_t n = 1;
        const size_t line = cfg.seq ? groups[(size_t)t].first : (size_t)t;
        if (cfg.seq && groups[(size_t)t].seq >= 0) n = run_sequence(ctx, cfg, pairs, groups[(size_t)t]);
        else run_line(ctx, cfg, pairs[line], line);
        std::lock_guard<std::mutex> lk(P.m); P.taken += n;
    }
}
