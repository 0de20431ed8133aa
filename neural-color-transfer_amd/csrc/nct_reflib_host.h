// nct_reflib_host.h — reference libraries (SPEC §6.21): the host object and the host-side rules, in plain C++ without the HIP runtime, so that nct_reflib.cpp and a
// stand-alone program under the host sanitizers (tests/reflib_host_check.cpp) compile the same text. A library is the tap, C, an optional centre and the int8 descriptor
// rows of its entries end to end with their offsets; rule D4 (the key and the order) is host arithmetic on the two sums the device returns.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#define NCT_REFLIB_MAX_ENTRIES 4096
#define NCT_REFLIB_MAX_ROWS 65536                 // per entry, and of the source: rule D1
#define NCT_REFLIB_MAX_BYTES (1LL << 31)          // all rows of a library

static const int kReflibTapC[5] = {64, 128, 256, 512, 512};

struct nct_reflib {
    int tap = 0, C = 0;
    bool centred = false;
    std::vector<float> center;                    // [C] with centred
    std::vector<int8_t> rows;                     // [offsets.back()][C]
    std::vector<int32_t> offsets{0};              // [N + 1]
    unsigned long long id = 0, revision = 0;      // what a context's device copy is keyed by: the object (ids are never reused) and a counter every add bumps
    int N() const { return (int)offsets.size() - 1; }
    long long total() const { return offsets.back(); }
};

// the refusal of a (tap, C) pair, or an empty string
static inline std::string reflib_tap_check(const char* who, int tap, int C) {
    char msg[160];
    if (tap < 1 || tap > 5) { snprintf(msg, sizeof msg, "%s: tap must be in [1, 5] (got %d)", who, tap); return msg; }
    if (C != kReflibTapC[tap - 1]) { snprintf(msg, sizeof msg, "%s: C must be %d at tap %d (got %d)", who, kReflibTapC[tap - 1], tap, C); return msg; }
    return "";
}

// the refusal of a row table (rows end to end, offsets [N + 1]), or an empty string: nct_descriptor_match's and nct_reflib_from_rows' limits
static inline std::string reflib_table_check(const char* who, int C, const void* rows, const int32_t* offsets, int N) {
    char msg[200];
    if (C < 16 || C > 4096 || (C & 15)) { snprintf(msg, sizeof msg, "%s: C must be a multiple of 16 in [16, 4096] (got %d)", who, C); return msg; }
    if (N < 1 || N > NCT_REFLIB_MAX_ENTRIES) { snprintf(msg, sizeof msg, "%s: N must be in [1, %d] (got %d)", who, NCT_REFLIB_MAX_ENTRIES, N); return msg; }
    if (!rows) { snprintf(msg, sizeof msg, "%s: null rows", who); return msg; }
    if (!offsets) { snprintf(msg, sizeof msg, "%s: null offsets", who); return msg; }
    if (offsets[0] != 0) { snprintf(msg, sizeof msg, "%s: offsets[0] must be 0 (got %d)", who, offsets[0]); return msg; }
    for (int k = 0; k < N; ++k) {
        const long long n = (long long)offsets[k + 1] - offsets[k];
        if (n < 1 || n > NCT_REFLIB_MAX_ROWS) { snprintf(msg, sizeof msg, "%s: offsets: entry %d must hold 1 to %d rows (got %lld)", who, k, NCT_REFLIB_MAX_ROWS, n); return msg; }
        if ((long long)offsets[k + 1] * C > NCT_REFLIB_MAX_BYTES) { snprintf(msg, sizeof msg, "%s: offsets: the rows up to entry %d exceed 2^31 bytes", who, k); return msg; }
    }
    return "";
}

// appends one entry's rows [n][C]; the refusal, or an empty string (the library is then unchanged)
static inline std::string reflib_append(nct_reflib& L, const char* who, const int8_t* rows, int n) {
    char msg[200];
    if (n < 1 || n > NCT_REFLIB_MAX_ROWS) { snprintf(msg, sizeof msg, "%s: the tap grid must hold 1 to %d cells (got %d)", who, NCT_REFLIB_MAX_ROWS, n); return msg; }
    if (L.N() >= NCT_REFLIB_MAX_ENTRIES) { snprintf(msg, sizeof msg, "%s: the library holds %d entries already", who, NCT_REFLIB_MAX_ENTRIES); return msg; }
    if ((L.total() + n) * L.C > NCT_REFLIB_MAX_BYTES) { snprintf(msg, sizeof msg, "%s: the library's rows would exceed 2^31 bytes", who); return msg; }
    L.rows.reserve(L.rows.size() + (size_t)n * L.C);
    L.offsets.reserve(L.offsets.size() + 1);      // both grow, or neither
    L.rows.insert(L.rows.end(), rows, rows + (size_t)n * L.C);
    L.offsets.push_back((int32_t)(L.total() + n));
    ++L.revision;
    return "";
}

static inline long long reflib_floor_div(long long a, long long b /* > 0 */) { const long long q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }

// rule D4: |fwd| <= na * 2^26 <= 2^42, so the product with 1024 stays in int64
static inline long long reflib_key(long long fwd, long long bwd, int na, int nb, int wf, int wb) {
    return wf * reflib_floor_div(fwd * 1024, na) + wb * reflib_floor_div(bwd * 1024, nb);
}

// descending key, the lower index first on a tie
static inline void reflib_order(const long long* key, int N, int32_t* order) {
    std::iota(order, order + N, 0);
    std::stable_sort(order, order + N, [&](int32_t x, int32_t y) { return key[x] > key[y]; });
}
