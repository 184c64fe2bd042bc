// hops_host_san_test.cpp -- rm_hops_from_links (radio-sim_amd/csrc/rm_api_hops.cpp), the pure host form of the hop query
// (extension E17), under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, no device is touched.
// tests/test_hops_ref.py compiles rm_api_hops.cpp beside this file with -fsanitize=address,undefined and runs it.
// Every array is a heap block of exactly the size the call may touch, so a write or a read one element beyond is reported.
// Checks, on random link lists: the tree's invariants (a parent is one level closer, over a listed link at or above the threshold,
// and no listed link at or above it is stronger or ties with a smaller index; no link leads from an unreached node to a reached
// one; children and totals add up), the optional outputs left out in turn, empty inputs, and every refusal.  Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "../../include/radiomedium_hip.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("failed at line %d: %s\n", __LINE__, #c);         \
            return 1;                                                     \
        }                                                                 \
    } while (0)

template <typename T> static std::unique_ptr<T[]> block(int n) { return std::unique_ptr<T[]>(n > 0 ? new T[size_t(n)] : nullptr); }

static int one(std::mt19937_64 &rng, int n, int m, int nr, double min_rssi, int leave_out)
{
    auto node = block<int32_t>(m), far = block<int32_t>(m), roots = block<int32_t>(nr);
    auto rssi = block<double>(m);
    for (int i = 0; i < m; ++i) {
        node[i] = int32_t(rng() % uint64_t(n));
        far[i] = int32_t(rng() % uint64_t(n));
        rssi[i] = (rng() % 17 == 0) ? std::numeric_limits<double>::quiet_NaN() : -95.0 + double(rng() % 40); // (ties are frequent)
    }
    for (int k = 0; k < nr; ++k) roots[k] = int32_t(rng() % uint64_t(n));
    auto hop = block<int32_t>(n), parent = block<int32_t>(n), children = block<int32_t>(n);
    auto prssi = block<double>(n);
    rm_hops_out out{hop.get(), leave_out == 1 ? nullptr : parent.get(), leave_out == 2 ? nullptr : prssi.get(), leave_out == 3 ? nullptr : children.get()};
    rm_hops_totals t{-7, -7, -7, -7};
    CHECK(rm_hops_from_links(n, m, node.get(), far.get(), rssi.get(), min_rssi, roots.get(), nr, &out, &t) == RM_OK);
    int reached = 0, max_hop = -1, n_roots = 0;
    for (int j = 0; j < n; ++j) {
        CHECK(hop[j] >= -1);
        reached += hop[j] >= 0;
        n_roots += hop[j] == 0;
        if (hop[j] > max_hop) max_hop = hop[j];
    }
    CHECK(t.reached == reached && t.max_hop == max_hop && t.roots == n_roots && t.reserved == 0);
    for (int k = 0; k < nr; ++k) CHECK(hop[roots[k]] == 0);
    auto is_link = [&](int i) { return node[i] != far[i] && rssi[i] >= min_rssi; };
    for (int i = 0; i < m; ++i) {
        if (!is_link(i)) continue;
        if (hop[far[i]] >= 0) CHECK(hop[node[i]] >= 0 && hop[node[i]] <= hop[far[i]] + 1); // (a level is never skipped)
    }
    if (leave_out != 0) return 0;
    auto count = block<int32_t>(n);
    for (int j = 0; j < n; ++j) count[j] = 0;
    for (int j = 0; j < n; ++j) {
        uint64_t bits;
        std::memcpy(&bits, &prssi[j], 8);
        if (hop[j] < 1) {
            CHECK(parent[j] == -1 && bits == 0x7FF8000000000000ull);
            continue;
        }
        const int p = parent[j];
        CHECK(p >= 0 && p < n && p != j && hop[p] == hop[j] - 1);
        ++count[p];
        bool listed = false;
        for (int i = 0; i < m; ++i) {
            if (!is_link(i) || node[i] != j || hop[far[i]] != hop[j] - 1) continue;
            listed = listed || (far[i] == p && rssi[i] == prssi[j]);
            CHECK(!(rssi[i] > prssi[j]) && !(rssi[i] == prssi[j] && far[i] < p)); // (no candidate precedes the parent)
        }
        CHECK(listed);
    }
    for (int j = 0; j < n; ++j) CHECK(children[j] == count[j]);
    return 0;
}

int main()
{
    std::mt19937_64 rng(17);
    const double inf = std::numeric_limits<double>::infinity();
    for (int rep = 0; rep < 300; ++rep) {
        const int n = 1 + int(rng() % 40), m = int(rng() % 200), nr = int(rng() % 4);
        const double min_rssi = rep % 5 == 0 ? -inf : rep % 5 == 1 ? inf : -95.0 + double(rng() % 30);
        if (one(rng, n, m, nr, min_rssi, rep % 4)) return 1;
    }
    // empty inputs
    rm_hops_out none{nullptr, nullptr, nullptr, nullptr};
    rm_hops_totals t{-7, -7, -7, -7};
    auto hop0 = block<int32_t>(1);
    rm_hops_out just{hop0.get(), nullptr, nullptr, nullptr};
    CHECK(rm_hops_from_links(0, 0, nullptr, nullptr, nullptr, -inf, nullptr, 0, &just, &t) == RM_OK && t.reached == 0 && t.max_hop == -1 && t.roots == 0);
    CHECK(rm_hops_from_links(1, 0, nullptr, nullptr, nullptr, -inf, nullptr, 0, &just, nullptr) == RM_OK && hop0[0] == -1);
    // refusals
    int32_t a[1] = {0}, bad_hi[1] = {1}, bad_lo[1] = {-1};
    double r[1] = {-50.0};
    CHECK(rm_hops_from_links(1, 1, a, a, r, -inf, a, 1, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, a, r, -inf, a, 1, &none, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(-1, 0, a, a, r, -inf, a, 0, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, -1, a, a, r, -inf, a, 0, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 0, a, a, r, -inf, a, -1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, nullptr, a, r, -inf, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, nullptr, r, -inf, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, a, nullptr, -inf, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, a, r, -inf, nullptr, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, a, r, std::nan(""), a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, bad_hi, a, r, -inf, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, bad_lo, r, -inf, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, a, r, -inf, bad_hi, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_hops_from_links(1, 1, a, a, r, -inf, bad_lo, 1, &just, nullptr) == RM_ERR_INVALID);
    std::printf("ok\n");
    return 0;
}
