// nct_wls_schedule.h — how many PCG iterations the S2 solver (k_wls_mg.hip: pcg_part) enqueues between two convergence polls. Plain host C++: it knows nothing of
// streams, events or the page-locked slots, so tests/wls_schedule_check.cpp drives it with a model solver on the CPU.
#pragma once
#include <cmath>

constexpr int WLS_BATCH = 2;      // iterations enqueued between two convergence polls (even: the state double buffer); 4: +1.0 ms of empty launches past convergence per pair, 6: +1.3

// Snapshot k is published by the last kernel of the k-th enqueue (k = 0: by the start kernel); the host reads them in order, one per turn, after it
// has enqueued the next batch. How MANY iterations that batch gets is a forecast: from the last two snapshots it has read, the host knows r.r of every
// system still iterating and its decay per iteration, hence the iterations still needed (the one that finds r.r below the threshold included); what is
// already in flight is subtracted. A forecast of 0 enqueues nothing and just waits for the in-flight snapshot — if the solve is not done then (the decay
// slowed down), the GPU idles for one host round trip (~20 us), about what ONE needless iteration costs, and the next batch comes from a fresh forecast; without
// the forecast every solve ran 2-4 needless iterations (22-44 empty launches: 19 iterations of 110 per 700x700 pair). The forecast never changes what an iteration computes.
struct WlsSchedule {
    const int nq, maxit; const bool use_forecast; const double rtol2;    // systems, iteration budget, NCT_WLS_FORECAST, rtol^2: set by the solver
    // the state: the solver reads it, only enqueued() and read() change it
    int it = 0;                                            // iterations enqueued
    int issued = 0, seen = -1;                             // snapshot numbers: the last one published by what is enqueued, the last one read
    int its_at_snapshot[2] = {0, 0};                       // iterations enqueued when snapshot (k & 1) was taken
    int its_seen = 0;                                      // ... when snapshot `seen` was taken: it - its_seen iterations are in flight behind it
    double prev_rho[6] = {}; int prev_its = -1;            // of the snapshot read before `seen`: its r.r and the iteration that saw them
    int remaining_after_seen = -1;                         // forecast: iterations still needed after snapshot `seen`; -1 = none
    int iters[6] = {};                                     // iteration counts of snapshot `seen`; final once done: iterations enqueued after it leave the state untouched (nactive == 0)
    bool done = false;                                     // every system has converged
    // Iterations to enqueue now; the last of them publishes snapshot issued + 1. 0: enqueue nothing, the turn only reads the snapshot in flight.
    int next_batch() const {
        int want = WLS_BATCH;
        if (use_forecast && remaining_after_seen >= 0) {
            want = remaining_after_seen - (it - its_seen);
            if (want > WLS_BATCH) want = WLS_BATCH;
            if (want < 0) want = 0;                        // only with iterations in flight: nothing in flight => want = need >= 1
        }
        if (it + want > maxit) want = maxit - it;
        return want;
    }
    void enqueued(int n) { if (n > 0) { it += n; ++issued; its_at_snapshot[issued & 1] = it; } }
    bool pending() const { return seen < issued; }        // a snapshot is left to read (false: the iteration budget is spent)
    // Takes snapshot seen + 1: any struct with the solver state's rho, bb, active, iters, nactive. true = stop: converged, or the budget is spent and nothing is in flight.
    template <class State> bool read(const State& fin) {
        ++seen; its_seen = its_at_snapshot[seen & 1];
        for (int q = 0; q < nq; ++q) iters[q] = fin.iters[q];
        if (fin.nactive == 0) { done = true; return true; }
        if (it >= maxit && seen == issued) return true;
        if (!use_forecast) return false;
        // iterations still needed after this snapshot: the slowest system's m = ceil(log(threshold / rho) / log(decay per iteration)), decay from the
        // previous snapshot read; no forecast (full batches) while there is no history or the residual does not decay
        const int ridx = its_seen > 0 ? its_seen - 1 : 0;   // fin.rho = r_ridx . r_ridx (the start kernel and iteration 0 both see r_0)
        int need = -1; bool ok = prev_its >= 0 && ridx > prev_its;
        if (ok) {
            need = 1;
            for (int q = 0; q < nq; ++q) {
                if (!fin.active[q]) continue;
                const double thr = rtol2 * fin.bb[q], rho = fin.rho[q];
                if (!(rho > 0.0) || !(prev_rho[q] > 0.0) || !(thr > 0.0)) { ok = false; break; }
                const double decay = pow(rho / prev_rho[q], 1.0 / (double)(ridx - prev_its));
                if (!(decay < 0.95)) { ok = false; break; }
                // fin.rho = r.r the LAST iteration saw, i.e. one update older than the residual now: the next iteration sees rho * decay
                const double m = rho * decay <= thr ? 1.0 : 1.0 + ceil(log(thr / (rho * decay)) / log(decay));
                if (m > need) need = (int)(m < 1e6 ? m : 1e6);
            }
        }
        remaining_after_seen = ok ? need : -1;
        for (int q = 0; q < nq; ++q) prev_rho[q] = fin.rho[q];
        prev_its = ridx;
        return false;
    }
};
