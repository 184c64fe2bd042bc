// routes_host_san_test.cpp -- rm_routes_from_links and rm_routes_link_cost (radio-sim_amd/csrc/rm_api_routes.cpp), the pure host
// forms of the route query (extension E18), under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, no device is
// touched.  tests/test_routes_ref.py compiles rm_api_routes.cpp beside this file with -fsanitize=address,undefined and runs it.
// Every array is a heap block of exactly the size the call may touch, so a write or a read one element beyond is reported.
// Checks, on random link lists: the costs are the least fixed point (roots 0; no counting link could lower a cost; every reached
// node that is no root has a parent whose cost plus the link's cost is its own, so the costs are attained; no counting link leads
// from an unreached node to a reached one), no candidate precedes the parent, link_cost / children / totals add up, the optional
// outputs left out in turn, rssi values from -inf to +inf and NaN, empty inputs, and every refusal.  Prints "ok".
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

static const double kNoise = -100.0;

static int one(std::mt19937_64 &rng, int n, int m, int nr, const rm_routes_params &prm, int leave_out)
{
    const double inf = std::numeric_limits<double>::infinity();
    auto node = block<int32_t>(m), far = block<int32_t>(m), roots = block<int32_t>(nr);
    auto rssi = block<double>(m);
    for (int i = 0; i < m; ++i) {
        node[i] = int32_t(rng() % uint64_t(n));
        far[i] = int32_t(rng() % uint64_t(n));
        const uint64_t pick = rng() % 23;
        // around the noise floor, where the cost moves from the cap to 128 (ties are frequent: half-dB steps)
        rssi[i] = pick == 0 ? std::numeric_limits<double>::quiet_NaN() : pick == 1 ? -inf : pick == 2 ? inf : -104.0 + 0.5 * double(rng() % 30);
    }
    for (int k = 0; k < nr; ++k) roots[k] = int32_t(rng() % uint64_t(n));
    auto cost = block<uint64_t>(n);
    auto parent = block<int32_t>(n), children = block<int32_t>(n);
    auto lc = block<uint32_t>(n);
    auto prssi = block<double>(n);
    rm_routes_out out{cost.get(), leave_out == 1 ? nullptr : parent.get(), leave_out == 2 ? nullptr : prssi.get(), leave_out == 3 ? nullptr : lc.get(),
                      leave_out == 4 ? nullptr : children.get()};
    rm_routes_totals t{-7, -7, 77};
    CHECK(rm_routes_from_links(n, m, node.get(), far.get(), rssi.get(), &prm, kNoise, roots.get(), nr, &out, &t) == RM_OK);
    int reached = 0, n_roots = 0;
    uint64_t max_cost = 0;
    for (int j = 0; j < n; ++j) {
        if (cost[j] == RM_ROUTE_UNREACHED) continue;
        ++reached;
        n_roots += cost[j] == 0;
        CHECK(cost[j] == 0 || cost[j] >= 128);
        if (cost[j] > max_cost) max_cost = cost[j];
    }
    CHECK(t.reached == reached && t.roots == n_roots && t.max_cost == max_cost);
    for (int k = 0; k < nr; ++k) CHECK(cost[roots[k]] == 0);
    auto link_c = block<uint32_t>(m); // 0: no counting link
    for (int i = 0; i < m; ++i) {
        uint32_t c = 0;
        link_c[i] = (node[i] != far[i] && rm_routes_link_cost(&prm, kNoise, rssi[i], &c)) ? c : 0u;
        if (!link_c[i]) continue;
        CHECK(c >= 128 && c <= prm.max_link_cost && rssi[i] >= prm.min_rssi_dbm);
        if (prm.kind == RM_EM_NONE) CHECK(c == 128);
        if (cost[far[i]] != RM_ROUTE_UNREACHED) CHECK(cost[node[i]] <= cost[far[i]] + c); // (nothing can be lowered, nobody is left out)
    }
    if (leave_out != 0) return 0;
    auto count = block<int32_t>(n);
    for (int j = 0; j < n; ++j) count[j] = 0;
    for (int j = 0; j < n; ++j) {
        uint64_t bits;
        std::memcpy(&bits, &prssi[j], 8);
        if (cost[j] == 0 || cost[j] == RM_ROUTE_UNREACHED) {
            CHECK(parent[j] == -1 && bits == 0x7FF8000000000000ull && lc[j] == 0);
            continue;
        }
        const int p = parent[j];
        CHECK(p >= 0 && p < n && p != j && cost[p] != RM_ROUTE_UNREACHED && cost[p] + lc[j] == cost[j]);
        ++count[p];
        bool listed = false;
        for (int i = 0; i < m; ++i) {
            if (!link_c[i] || node[i] != j || cost[far[i]] == RM_ROUTE_UNREACHED || cost[far[i]] + link_c[i] != cost[j]) continue;
            listed = listed || (far[i] == p && rssi[i] == prssi[j] && link_c[i] == lc[j]);
            CHECK(!(rssi[i] > prssi[j]) && !(rssi[i] == prssi[j] && far[i] < p)); // (no candidate precedes the parent)
        }
        CHECK(listed);
    }
    for (int j = 0; j < n; ++j) CHECK(children[j] == count[j]);
    return 0;
}

int main()
{
    std::mt19937_64 rng(18);
    const double inf = std::numeric_limits<double>::infinity();
    const rm_routes_params base{RM_NB_HEARD_BY, RM_EM_OQPSK_250K, 4.0, 4064, -inf, 1024, 0};
    for (int rep = 0; rep < 300; ++rep) {
        const int n = 1 + int(rng() % 40), m = int(rng() % 200), nr = int(rng() % 4);
        rm_routes_params p = base;
        p.kind = rep % 3 == 0 ? RM_EM_NONE : RM_EM_OQPSK_250K;
        p.min_rssi_dbm = rep % 7 == 0 ? inf : rep % 7 == 1 ? -101.5 : -inf;
        p.max_link_cost = rep % 11 == 0 ? 128u : rep % 11 == 1 ? 65535u : 1024u;
        p.air_us = rep % 13 == 0 ? 0 : 4064;
        if (one(rng, n, m, nr, p, rep % 5)) return 1;
    }
    // the link cost alone
    uint32_t c = 0;
    rm_routes_params none = base;
    none.kind = RM_EM_NONE;
    CHECK(rm_routes_link_cost(&none, kNoise, -94.0, &c) == 1 && c == 128);
    CHECK(rm_routes_link_cost(&none, kNoise, -94.0, nullptr) == 1);
    CHECK(rm_routes_link_cost(&base, kNoise, -60.0, &c) == 1 && c == 128);
    CHECK(rm_routes_link_cost(&base, kNoise, -inf, &c) == 0);
    CHECK(rm_routes_link_cost(&base, kNoise, std::nan(""), &c) == 0);
    CHECK(rm_routes_link_cost(&base, std::nan(""), -60.0, &c) == 0);
    CHECK(rm_routes_link_cost(nullptr, kNoise, -60.0, &c) == 0);
    // empty inputs
    rm_routes_out nothing{nullptr, nullptr, nullptr, nullptr, nullptr};
    rm_routes_totals t{-7, -7, 77};
    auto cost0 = block<uint64_t>(1);
    rm_routes_out just{cost0.get(), nullptr, nullptr, nullptr, nullptr};
    CHECK(rm_routes_from_links(0, 0, nullptr, nullptr, nullptr, &base, kNoise, nullptr, 0, &just, &t) == RM_OK && t.reached == 0 && t.roots == 0 && t.max_cost == 0);
    CHECK(rm_routes_from_links(1, 0, nullptr, nullptr, nullptr, &base, kNoise, nullptr, 0, &just, nullptr) == RM_OK && cost0[0] == RM_ROUTE_UNREACHED);
    // refusals
    int32_t a[1] = {0}, bad_hi[1] = {1}, bad_lo[1] = {-1};
    double r[1] = {-50.0};
    CHECK(rm_routes_from_links(1, 1, a, a, r, &base, kNoise, a, 1, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, a, r, &base, kNoise, a, 1, &nothing, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, a, r, nullptr, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(-1, 0, a, a, r, &base, kNoise, a, 0, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, -1, a, a, r, &base, kNoise, a, 0, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 0, a, a, r, &base, kNoise, a, -1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, nullptr, a, r, &base, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, nullptr, r, &base, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, a, nullptr, &base, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, a, r, &base, kNoise, nullptr, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, bad_hi, a, r, &base, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, bad_lo, r, &base, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, a, r, &base, kNoise, bad_hi, 1, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_routes_from_links(1, 1, a, a, r, &base, kNoise, bad_lo, 1, &just, nullptr) == RM_ERR_INVALID);
    for (int k = 0; k < 9; ++k) {
        rm_routes_params p = base;
        if (k == 0) p.kind = 2;
        if (k == 1) p.reserved = 1;
        if (k == 2) p.us_per_bit = 0.0;
        if (k == 3) p.us_per_bit = inf;
        if (k == 4) p.us_per_bit = std::nan("");
        if (k == 5) p.air_us = -1;
        if (k == 6) p.min_rssi_dbm = std::nan("");
        if (k == 7) p.max_link_cost = 127;
        if (k == 8) p.max_link_cost = 65536;
        CHECK(rm_routes_from_links(1, 1, a, a, r, &p, kNoise, a, 1, &just, nullptr) == RM_ERR_INVALID);
        CHECK(rm_routes_link_cost(&p, kNoise, -60.0, &c) == 0);
    }
    std::printf("ok\n");
    return 0;
}
