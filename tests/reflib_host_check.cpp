// reflib_host_check.cpp — runs csrc/nct_reflib_host.h (the host object of reference libraries and rule D4 of SPEC §6.21) as text, so that tests/test_reflib.py can hold it
// against tests/reflib_ref.py and run it under the host sanitizers: no GPU, no HIP runtime. Stdin, one case per line:
//   table C N o_0 … o_N          -> "ok" or the refusal of reflib_table_check; with "ok" the library built entry by entry with reflib_append: "lib N total revision o_0 … o_N sum"
//                                   (sum: the sum of all row bytes read back through the object, every row of entry k filled with k + 1 - 3 (c % 7))
//   tap T C                      -> "ok" or the refusal of reflib_tap_check
//   rank na wf wb N (fwd bwd nb) x N -> "key k_0 … order o_0 …"
#include "nct_reflib_host.h"
#include <iostream>
#include <sstream>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "tap") {
            int tap, C;
            in >> tap >> C;
            const std::string why = reflib_tap_check("check", tap, C);
            std::cout << (why.empty() ? "ok" : why) << "\n";
        } else if (what == "table") {
            int C, N;
            in >> C >> N;
            std::vector<int32_t> off;
            for (long long v; in >> v;) off.push_back((int32_t)v);
            std::vector<int8_t> dummy(16);
            const bool sized = N >= 0 && (int)off.size() == N + 1;
            const std::string why = reflib_table_check("check", C, dummy.data(), sized ? off.data() : nullptr, N);
            if (!why.empty()) { std::cout << why << "\n"; continue; }
            nct_reflib L;
            L.C = C;
            for (int k = 0; k < N; ++k) {
                const int n = off[k + 1] - off[k];
                std::vector<int8_t> rows((size_t)n * C);
                for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int8_t)(k + 1 - 3 * (int)((i % C) % 7));
                const std::string bad = reflib_append(L, "check", rows.data(), n);
                if (!bad.empty()) { std::cout << bad << "\n"; break; }
            }
            // refused appends leave the object as it was
            std::vector<int8_t> one((size_t)C);
            const std::string r0 = reflib_append(L, "check", one.data(), 0), r1 = reflib_append(L, "check", one.data(), NCT_REFLIB_MAX_ROWS + 1);
            long long sum = 0;
            for (int8_t v : L.rows) sum += v;
            std::cout << "lib " << L.N() << " " << L.total() << " " << L.revision;
            for (int32_t o : L.offsets) std::cout << " " << o;
            std::cout << " " << sum << " " << (r0.empty() || r1.empty() ? "append-not-refused" : "refusals-ok") << "\n";
        } else if (what == "rank") {
            int na, wf, wb, N;
            in >> na >> wf >> wb >> N;
            std::vector<long long> key((size_t)N);
            for (int k = 0; k < N; ++k) {
                long long f, b; int nb;
                in >> f >> b >> nb;
                key[k] = reflib_key(f, b, na, nb, wf, wb);
            }
            std::vector<int32_t> order((size_t)N);
            reflib_order(key.data(), N, order.data());
            std::cout << "key";
            for (long long k : key) std::cout << " " << k;
            std::cout << " order";
            for (int32_t o : order) std::cout << " " << o;
            std::cout << "\n";
        }
    }
    return 0;
}
