// etx_host_san_test.cpp -- rm_etx_from_tables, rm_etx_link_cost and rm_etx_combine (radio-sim_amd/csrc/rm_api_etx.cpp), the pure
// host forms of the measured-route query (extension E21), under AddressSanitizer + UndefinedBehaviorSanitizer: host code only, no
// device is touched.  tests/test_etx_ref.py compiles rm_api_etx.cpp beside this file with -fsanitize=address,undefined and runs it.
// Every array is a heap block of exactly the size the call may touch, so a write or a read one element beyond is reported.
// Checks, on random tables with junk peers: the costs are the least fixed point (roots 0; no counting link could lower a cost;
// every reached node that is no root has a parent with a strictly smaller cost whose cost plus the link's is within the
// hysteresis, and exactly its own when the parent is not the current one; no counting link leads from an unreached node to a
// reached one), slot / link_cost / children / totals add up, cur as the parent array itself, the optional outputs left out in turn,
// empty inputs, and every refusal.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
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

template <typename T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(n > 0 ? new T[n] : nullptr); }

// c(j, k) by the public pieces alone; 0: the link does not count
static uint32_t link(int n, int K, const int32_t *peer, const rm_link_stats *st, const rm_etx_params &p, int j, int k)
{
    const int32_t q = peer[size_t(j) * K + k];
    uint32_t c = 0, r = 0;
    if (q < 0 || q >= n || q == j || !rm_etx_link_cost(&p, st[size_t(j) * K + k].heard, st[size_t(j) * K + k].delivered, &c)) return 0;
    if (p.mode == RM_ETX_INBOUND) return c;
    for (int s = 0; s < K; ++s)
        if (peer[size_t(q) * K + s] == j) {
            if (!rm_etx_link_cost(&p, st[size_t(q) * K + s].heard, st[size_t(q) * K + s].delivered, &r)) return 0;
            const uint64_t both = rm_etx_combine(c, r);
            return both <= p.max_link_cost ? uint32_t(both) : 0;
        }
    return 0;
}

static int one(std::mt19937_64 &rng, int n, int K, int nr, const rm_etx_params &prm, int leave_out, bool with_cur, bool alias)
{
    const size_t nk = size_t(n) * size_t(K);
    auto peer = block<int32_t>(nk), roots = block<int32_t>(size_t(nr));
    auto st = block<rm_link_stats>(nk);
    for (size_t i = 0; i < nk; ++i) {
        const uint64_t pick = rng() % 16;
        peer[i] = pick == 0 ? -1 : pick == 1 ? n : pick == 2 ? INT32_MAX : pick == 3 ? INT32_MIN : int32_t(rng() % uint64_t(n));
        std::memset(&st[i], 0, sizeof(rm_link_stats));
        st[i].heard = rng() % 50;
        st[i].delivered = rng() % 11 == 0 ? st[i].heard + 3 : rng() % (st[i].heard + 1);
    }
    for (int k = 0; k < nr; ++k) roots[k] = int32_t(rng() % uint64_t(n));
    auto cost = block<uint64_t>(size_t(n));
    auto parent = block<int32_t>(size_t(n)), slot = block<int32_t>(size_t(n)), children = block<int32_t>(size_t(n)), cur = block<int32_t>(size_t(n));
    auto lc = block<uint32_t>(size_t(n));
    for (int j = 0; j < n; ++j) cur[j] = rng() % 5 == 0 ? -1 : int32_t(rng() % uint64_t(n + 2));
    if (alias) std::memcpy(parent.get(), cur.get(), size_t(n) * 4);
    const rm_etx_tables tb{peer.get(), st.get(), K, 0};
    rm_etx_out out{cost.get(), leave_out == 1 ? nullptr : parent.get(), leave_out == 2 ? nullptr : slot.get(), leave_out == 3 ? nullptr : lc.get(),
                   leave_out == 4 ? nullptr : children.get()};
    rm_etx_totals t{-7, -7, -7, -7, -7, -7, 77};
    const int32_t *cur_arg = !with_cur ? nullptr : (alias && out.parent) ? out.parent : cur.get();
    CHECK(rm_etx_from_tables(n, &tb, &prm, roots.get(), nr, cur_arg, &out, &t) == RM_OK);
    int reached = 0, n_roots = 0;
    uint64_t max_cost = 0;
    for (int j = 0; j < n; ++j) {
        if (cost[j] == RM_ROUTE_UNREACHED) continue;
        ++reached;
        n_roots += cost[j] == 0;
        CHECK(cost[j] == 0 || cost[j] >= 128);
        if (cost[j] > max_cost) max_cost = cost[j];
    }
    CHECK(t.reached == reached && t.roots == n_roots && t.max_cost == max_cost && t.reserved == 0);
    for (int k = 0; k < nr; ++k) CHECK(cost[roots[k]] == 0);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < K; ++k) {
            const uint32_t c = link(n, K, peer.get(), st.get(), prm, j, k);
            if (!c) continue;
            CHECK(c >= 128 && c <= prm.max_link_cost);
            const int32_t q = peer[size_t(j) * K + k];
            if (cost[q] != RM_ROUTE_UNREACHED) CHECK(cost[j] <= cost[q] + c); // (nothing can be lowered, nobody is left out)
        }
    if (leave_out != 0) return 0;
    auto count = block<int32_t>(size_t(n));
    for (int j = 0; j < n; ++j) count[j] = 0;
    int kept = 0, switched = 0, lost = 0;
    for (int j = 0; j < n; ++j) {
        const bool valid = with_cur && cur[j] >= 0 && cur[j] < n;
        if (cost[j] == 0 || cost[j] == RM_ROUTE_UNREACHED) {
            CHECK(parent[j] == -1 && slot[j] == -1 && lc[j] == 0);
            lost += cost[j] != 0 && valid;
            continue;
        }
        const int p = parent[j];
        CHECK(p >= 0 && p < n && p != j && slot[j] >= 0 && slot[j] < K && peer[size_t(j) * K + slot[j]] == p);
        CHECK(lc[j] == link(n, K, peer.get(), st.get(), prm, j, slot[j]) && lc[j] != 0);
        CHECK(cost[p] < cost[j]); // (loop-free for every hysteresis)
        if (valid && p == cur[j]) CHECK(cost[p] + lc[j] <= cost[j] + prm.hysteresis);
        else CHECK(cost[p] + lc[j] == cost[j]);
        kept += valid && p == cur[j];
        switched += valid && p != cur[j];
        ++count[p];
    }
    for (int j = 0; j < n; ++j) CHECK(children[j] == count[j]);
    CHECK(t.kept == kept && t.switched == switched && t.lost == lost);
    return 0;
}

int main()
{
    std::mt19937_64 rng(21);
    rm_etx_params base;
    rm_etx_defaults(&base);
    CHECK(base.mode == RM_ETX_INBOUND && base.min_heard == 4 && base.max_link_cost == 2048 && base.hysteresis == 192 && base.reserved == 0 && base.reserved2 == 0);
    CHECK(rm_etx_validate(&base) == RM_OK && rm_etx_validate(nullptr) == RM_ERR_INVALID);
    const int Ks[4] = {1, 2, 4, 8};
    for (int rep = 0; rep < 400; ++rep) {
        const int n = 1 + int(rng() % 40), K = Ks[rep % 4], nr = int(rng() % 4);
        rm_etx_params p = base;
        p.mode = (rep / 4) % 2;
        p.min_heard = rep % 7 == 0 ? 0u : rep % 7 == 1 ? 20u : 4u;
        p.max_link_cost = rep % 11 == 0 ? 128u : rep % 11 == 1 ? 65535u : 1024u;
        p.hysteresis = rep % 3 == 0 ? 0u : rep % 3 == 1 ? 192u : 65535u;
        if (one(rng, n, K, nr, p, rep % 5, rep % 2 == 0, rep % 4 == 0)) return 1;
    }
    // the entry cost alone
    uint32_t c = 0;
    CHECK(rm_etx_link_cost(&base, 40, 40, &c) == 1 && c == 128);
    CHECK(rm_etx_link_cost(&base, 40, 40, nullptr) == 1);
    CHECK(rm_etx_link_cost(&base, 40, 30, &c) == 1 && c == 171);
    CHECK(rm_etx_link_cost(&base, 3, 3, &c) == 0 && rm_etx_link_cost(&base, 40, 0, &c) == 0);
    CHECK(rm_etx_link_cost(&base, 1ull << 40, 1ull << 40, &c) == 1 && c == 128);
    CHECK(rm_etx_link_cost(&base, (1ull << 40) + 1, 1ull << 40, &c) == 0);
    CHECK(rm_etx_link_cost(&base, 10, UINT64_MAX, &c) == 1 && c == 128);
    CHECK(rm_etx_link_cost(nullptr, 40, 40, &c) == 0);
    CHECK(rm_etx_combine(128, 128) == 128 && rm_etx_combine(512, 500) == 2000 && rm_etx_combine(UINT32_MAX, UINT32_MAX) == ((uint64_t(UINT32_MAX) * UINT32_MAX + 64) >> 7));
    // empty inputs
    rm_etx_totals t{-7, -7, -7, -7, -7, -7, 77};
    auto cost0 = block<uint64_t>(1);
    auto peer0 = block<int32_t>(1);
    auto st0 = block<rm_link_stats>(1);
    peer0[0] = 0;
    std::memset(st0.get(), 0, sizeof(rm_link_stats));
    const rm_etx_tables tb{peer0.get(), st0.get(), 1, 0};
    rm_etx_out nothing{nullptr, nullptr, nullptr, nullptr, nullptr};
    rm_etx_out just{cost0.get(), nullptr, nullptr, nullptr, nullptr};
    CHECK(rm_etx_from_tables(0, &tb, &base, nullptr, 0, nullptr, &just, &t) == RM_OK && t.reached == 0 && t.roots == 0 && t.max_cost == 0 && t.kept == 0);
    CHECK(rm_etx_from_tables(1, &tb, &base, nullptr, 0, nullptr, &just, nullptr) == RM_OK && cost0[0] == RM_ROUTE_UNREACHED);
    // refusals
    int32_t a[1] = {0}, bad_hi[1] = {1}, bad_lo[1] = {-1};
    CHECK(rm_etx_from_tables(1, &tb, &base, a, 1, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, &tb, &base, a, 1, nullptr, &nothing, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, &tb, nullptr, a, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, nullptr, &base, a, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(-1, &tb, &base, a, 0, nullptr, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, &tb, &base, a, -1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, &tb, &base, nullptr, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, &tb, &base, bad_hi, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    CHECK(rm_etx_from_tables(1, &tb, &base, bad_lo, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    for (int k = 0; k < 6; ++k) {
        rm_etx_tables bt = tb;
        if (k == 0) bt.K = 0;
        if (k == 1) bt.K = 3;
        if (k == 2) bt.K = 16;
        if (k == 3) bt.reserved = 1;
        if (k == 4) bt.peer = nullptr;
        if (k == 5) bt.stats = nullptr;
        CHECK(rm_etx_from_tables(1, &bt, &base, a, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
    }
    for (int k = 0; k < 8; ++k) {
        rm_etx_params p = base;
        if (k == 0) p.mode = 2;
        if (k == 1) p.mode = -1;
        if (k == 2) p.reserved = 1;
        if (k == 3) p.reserved2 = 1;
        if (k == 4) p.min_heard = (1u << 31) + 1u;
        if (k == 5) p.max_link_cost = 127;
        if (k == 6) p.max_link_cost = 65536;
        if (k == 7) p.hysteresis = 65536;
        CHECK(rm_etx_validate(&p) == RM_ERR_INVALID);
        CHECK(rm_etx_from_tables(1, &tb, &p, a, 1, nullptr, &just, nullptr) == RM_ERR_INVALID);
        CHECK(rm_etx_link_cost(&p, 40, 40, &c) == 0);
    }
    rm_etx_params edge = base;
    edge.min_heard = 1u << 31;
    edge.max_link_cost = 65535;
    edge.hysteresis = 65535;
    CHECK(rm_etx_validate(&edge) == RM_OK);
    std::printf("ok\n");
    return 0;
}
