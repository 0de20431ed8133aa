// wls_schedule_check.cpp — drives csrc/nct_wls_schedule.h (the batch schedule of the S2 PCG) with a model solver and compares the sequence of batch sizes,
// the iterations enqueued / needed and the snapshots read with the values the loop of pcg_part gave before the schedule became a class (tests/test_wls_schedule.py
// builds this with AddressSanitizer + UBSan). Exit status 0 and "ok <cases>" if every case matches.
#include "nct_wls_schedule.h"
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

// The solver as the schedule sees it (k_pcg_start_fin / k_cg_update): system q is active until the first iteration i whose r.r, rho(q, i), is <= rtol^2 * bb[q];
// rho[q] = the value of the last iteration the system took part in, or the one that found it converged; iters[q] = its active iterations. n = 0: the start kernel, which sees rho(q, 0).
struct Snapshot { double rho[6], bb[6]; int active[6], iters[6], nactive; };     // the fields of the solver state (PState) that the schedule reads
struct Model {
    int nq; double bb[6]; std::function<double(int, int)> rho; double rtol2;
    mutable int searched[6] = {0, 0, 0, 0, 0, 0};                        // iterations 0 .. searched[q] - 1 did not find system q converged (memo: after() is called with growing n)
    Snapshot after(int n) const {
        Snapshot s = {};
        for (int q = 0; q < nq; ++q) {
            const double thr = rtol2 * bb[q];
            while (searched[q] < n && rho(q, searched[q]) > thr) ++searched[q];
            const int c = searched[q] < n ? searched[q] : n;             // c < n: iteration c found the system converged
            s.bb[q] = bb[q]; s.iters[q] = c;
            s.active[q] = n == 0 ? rho(q, 0) > thr : c == n;
            s.rho[q] = rho(q, c < n || n == 0 ? c : n - 1);
            s.nactive += s.active[q];
        }
        return s;
    }
};
struct Run { std::vector<int> batches; int enqueued, needed, snapshots; bool converged; };

// pcg_part's loop with the launches left out
static Run drive(const Model& m, int maxit, bool forecast, int* bad_turns) {
    WlsSchedule sched{m.nq, maxit, forecast, m.rtol2};
    std::vector<Snapshot> published = {m.after(0)};
    Run r;
    while (true) {
        const int want = sched.next_batch();
        if (sched.it == sched.its_seen && sched.remaining_after_seen >= 0 && want < 1) ++*bad_turns;      // nothing in flight => want = need >= 1
        r.batches.push_back(want);
        if (want > 0) published.push_back(m.after(sched.it + want));
        sched.enqueued(want);
        if (!sched.pending()) break;
        if (sched.read(published[sched.seen + 1])) break;
    }
    r.enqueued = sched.it; r.snapshots = sched.seen + 1; r.converged = sched.done; r.needed = 0;
    for (int q = 0; q < m.nq; ++q) r.needed = sched.iters[q] > r.needed ? sched.iters[q] : r.needed;
    return r;
}

static std::vector<int> seq(std::initializer_list<std::pair<int, int>> runs) {       // {{count, value}, ...}
    std::vector<int> v; for (auto& p : runs) v.insert(v.end(), p.first, p.second); return v;
}
static Model geometric(int nq, double d, double spread = 0.02) {                         // rho(q, i) = (d (1 + spread q))^i, bb = 1
    return {nq, {1, 1, 1, 1, 1, 1}, [=](int q, int i) { return pow(d * (1.0 + spread * q), i); }, 3e-8 * 3e-8};
}
static Model stalling(double d, int at, double then) {                                    // 3 systems: d^i until i = at, then x `then` per iteration
    return {3, {1, 1, 1, 1, 1, 1}, [=](int q, int i) { return i <= at ? pow(d * (1.0 + 0.02 * q), i) : pow(d * (1.0 + 0.02 * q), at) * pow(then, i - at); }, 3e-8 * 3e-8};
}

int main() {
    struct Case { std::string name; Model m; int maxit; bool forecast; Run want; };
    Model zero = geometric(6, 0.1); zero.rho = [](int, int) { return 0.0; };
    Model two_zero = geometric(6, 0.1, 0.0); two_zero.bb[1] = two_zero.bb[4] = 0.0;
    { auto g = two_zero.rho; two_zero.rho = [g](int q, int i) { return q == 1 || q == 4 ? 0.0 : g(q, i); }; }
    Model one_slow = geometric(6, 0.1, 0.0);
    one_slow.rho = [](int q, int i) { return pow(q == 2 ? 0.3 : 0.1, i); };
    const std::vector<Case> cases = {
        {"d=0.01", geometric(6, 0.01), 5000, true, {{2, 2, 2, 2, 1, 0}, 9, 8, 6, true}},
        {"d=0.05", geometric(6, 0.05), 5000, true, {seq({{6, 2}, {1, 1}, {1, 0}}), 13, 12, 8, true}},
        {"d=0.10", geometric(6, 0.10), 5000, true, {seq({{8, 2}, {1, 1}, {1, 0}}), 17, 16, 10, true}},
        {"d=0.20", geometric(6, 0.20), 5000, true, {seq({{12, 2}, {1, 0}}), 24, 23, 13, true}},
        {"d=0.50", geometric(6, 0.50), 5000, true, {seq({{29, 2}, {1, 1}, {1, 0}}), 59, 58, 31, true}},
        {"d=0.01 fixed", geometric(6, 0.01), 5000, false, {seq({{6, 2}}), 12, 8, 6, true}},
        {"d=0.10 fixed", geometric(6, 0.10), 5000, false, {seq({{10, 2}}), 20, 16, 10, true}},
        {"d=0.50 fixed", geometric(6, 0.50), 5000, false, {seq({{31, 2}}), 62, 58, 31, true}},
        {"x0 solves", zero, 5000, true, {{2}, 2, 0, 1, true}},
        {"x0 solves fixed", zero, 5000, false, {{2}, 2, 0, 1, true}},
        {"0.01 then x0.3", stalling(0.01, 7, 0.3), 5000, true, {{2, 2, 2, 2, 1, 0, 2}, 11, 10, 7, true}},
        {"0.01 then x0.5", stalling(0.01, 7, 0.5), 5000, true, {{2, 2, 2, 2, 1, 0, 2, 1}, 12, 11, 8, true}},
        {"0.5 then x0.05", stalling(0.5, 6, 0.05), 5000, true, {seq({{9, 2}, {1, 0}}), 18, 17, 10, true}},
        {"two zero systems", two_zero, 5000, true, {seq({{8, 2}, {1, 1}, {1, 0}}), 17, 16, 10, true}},
        {"one slow system", one_slow, 5000, true, {seq({{15, 2}, {1, 0}}), 30, 29, 16, true}},
        {"maxit=4", geometric(6, 0.5, 0.0), 4, true, {{2, 2, 0}, 4, 4, 3, false}},
        {"maxit=4 fixed", geometric(6, 0.5, 0.0), 4, false, {{2, 2, 0}, 4, 4, 3, false}},
        {"maxit=5", geometric(6, 0.5, 0.0), 5, true, {{2, 2, 1, 0}, 5, 5, 4, false}},
        {"maxit=5 fixed", geometric(6, 0.5, 0.0), 5, false, {{2, 2, 1, 0}, 5, 5, 4, false}},
    };
    int failed = 0, bad_turns = 0;
    for (const Case& c : cases) {
        const Run r = drive(c.m, c.maxit, c.forecast, &bad_turns);
        if (r.batches == c.want.batches && r.enqueued == c.want.enqueued && r.needed == c.want.needed && r.snapshots == c.want.snapshots && r.converged == c.want.converged) continue;
        ++failed;
        printf("%s: batches", c.name.c_str()); for (int b : r.batches) printf(" %d", b);
        printf(", %d / %d / %d%s; expected %d / %d / %d\n", r.enqueued, r.needed, r.snapshots, r.converged ? "" : ", not converged", c.want.enqueued, c.want.needed, c.want.snapshots);
    }
    // the invariant that replaced the fixed-batch fall-back, over decays, stall points and stall rates (a short forecast shows as a 0 batch with iterations in flight, never as one without)
    int zero_batches = 0;
    for (double d = 0.01; d < 0.96; d += 0.06) for (int at = 1; at <= 40; at += 4) for (double then = 0.02; then < 0.9; then += 0.12) {
        const Run r = drive(stalling(d, at, then), 5000, true, &bad_turns);
        for (int b : r.batches) zero_batches += b == 0;
    }
    if (bad_turns) printf("%d turns with nothing in flight, a forecast and an empty batch\n", bad_turns);
    if (!zero_batches) printf("the sweep never met a forecast of 0\n");
    if (failed || bad_turns || !zero_batches) return 1;
    printf("ok %zu\n", cases.size());
    return 0;
}
