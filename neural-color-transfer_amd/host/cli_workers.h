// The driver's threads: which pairs.txt lines this process runs (Tickets), the bounded hand-over between the I/O pool and the GPU workers (Pipeline), and the loops.
#pragma once
#include <fcntl.h>
#include <unistd.h>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include "cli_job.h"

// Which pairs.txt lines this process runs. One process (-world 1): all of them, in order. One process per GPU (-world N -rank r; what `-procs N` forks): line i belongs to
// rank i mod N — or, with -steal 1, to whichever rank draws it: a counter in <output>/.tickets, advanced under an fcntl lock, hands the lines out in order to whoever is
// free (BASELINE config 5, mixed sizes; north_star's "work-stealing" — a file lock rather than RCCL: the ranks exchange one integer per pair, and a lock file also works
// between ranks that were started by hand on different devices, with no rendezvous). Which rank runs a pair has no influence on its result.
struct Tickets {
    size_t total = 0, next = 0; int rank = 0, world = 1, fd = -1;
    long draw() {                                                // next global line index, -1 when there is none left for this process
        if (fd >= 0) {
            struct flock lk; memset(&lk, 0, sizeof lk); lk.l_type = F_WRLCK; lk.l_whence = SEEK_SET;
            if (fcntl(fd, F_SETLKW, &lk) != 0) return -1;
            unsigned long long v = 0;
            if (pread(fd, &v, sizeof v, 0) != (ssize_t)sizeof v) v = 0;
            const long got = v < total ? (long)v : -1;
            if (got >= 0) { ++v; if (pwrite(fd, &v, sizeof v, 0) != (ssize_t)sizeof v) { /* the lock is released below; the next reader sees the old value and redoes the line: harmless */ } }
            lk.l_type = F_UNLCK; (void)fcntl(fd, F_SETLK, &lk);
            return got;
        }
        while (next < total && (int)(next % (size_t)world) != rank) ++next;
        return next < total ? (long)next++ : -1;
    }
};

// Bounded hand-over between the I/O pool and the GPU workers. `ready` holds decoded pairs (at most `cap`: the decoders stay a little ahead of the GPUs, not a
// whole batch), `results` finished ones waiting for the PNG encoder (the same bound: a worker blocks rather than pile up results if zlib falls behind).
struct Pipeline {
    std::mutex m; std::condition_variable cv;
    std::deque<std::unique_ptr<Job>> ready, results;
    Tickets tickets;                                             // drawn under m
    size_t cap = 4, taken = 0, loading = 0, finished = 0;        // taken: the lines this process has taken on
    bool exhausted = false;                                      // the ticket source has nothing left for this process
    // decoded pixels waiting for a GPU worker: images are queued BEFORE the GPU-side shrink to MAX_SIZE and a decoder accepts up to 64 MP (192 MB), so the queue is
    // bounded by bytes as well as by count — a new load starts only while the decoded backlog is below byte_cap (or nothing at all is queued or loading)
    // Loads in flight are charged too: a load reserves `load_estimate` bytes when it starts — the largest decoded pair seen so far, at least two 1000 x 1000
    // images — and is corrected to its real size when it lands in `ready`, so several I/O threads cannot all pass the test while the backlog is still being decoded.
    // Results waiting for the encoder are charged as well (`results_bytes`): with -fullres 1 an output has the content image's own size, up to 192 MB.
    size_t ready_bytes = 0, byte_cap = (size_t)1 << 30, loading_bytes = 0, load_estimate = (size_t)6 << 20, results_bytes = 0;
    bool may_load() const { return !exhausted && ready.size() + loading < cap && (ready_bytes + loading_bytes + results_bytes < byte_cap || ready.size() + loading == 0); }
    bool loads_done() const { return exhausted && loading == 0; }
    bool all_done() const { return exhausted && finished == taken; }
};

void io_thread(Pipeline& P, const Config& cfg, const std::vector<Pair>& pairs);      // the pool: decodes the lines it draws, encodes what the GPU workers finished
void gpu_worker(Pipeline& P, nct_ctx* ctx, const Config& cfg);                       // runs what the pool decoded
// a worker that serves itself (-io 0, -seq 1): it draws a ticket and decodes, runs and encodes it. With -seq 1 the ticket is a group — a whole sequence, whose
// lines it runs in file order, or one line of another kind — for -gpus, -inflight, -world, -steal and -procs alike; otherwise a pairs.txt line
void self_serving_worker(Pipeline& P, nct_ctx* ctx, const Config& cfg, const std::vector<Pair>& pairs, const std::vector<Group>& groups);
