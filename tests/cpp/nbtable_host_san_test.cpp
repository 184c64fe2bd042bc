// nbtable_host_san_test.cpp -- rm_nbtable_from_result, rm_nbtable_expire_tables, rm_nbtable_validate and rm_nbtable_defaults
// (radio-sim_amd/csrc/rm_api_nbtable.cpp), the pure host forms of the neighbour tables (extension E22), under AddressSanitizer +
// UndefinedBehaviorSanitizer: host code only, no device is touched.  tests/test_nbtable_ref.py compiles rm_api_nbtable.cpp beside
// this file with -fsanitize=address,undefined and runs it.  Every array is a heap block of exactly the size the call may touch, so
// a write or a read one element beyond is reported.
// Checks, on random results (junk sources and receivers, NaN / infinite / huge rssi, empty packets, pkt_rssi instead of rssi) over
// random tables (junk peers, huge counters, INT64 extremes): a row's valid entries stay distinct; at most one slot per row changes
// and only in a row with a heard link; the counters add up to the totals, admitted >= evicted_stale + evicted_poor; a pinned slot
// is never replaced; the fresh entry's heard is the number of the slot's links from the admitted sender to that receiver; the
// expire walk empties exactly the slots that are held, not pinned and stale; empty inputs; every refusal.  Prints "ok".
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

template <typename T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(n > 0 ? new T[n] : nullptr); }

static bool held(int n, int d, int32_t v) { return v >= 0 && v < n && v != d; }
static bool stale(const rm_nbtable_params &p, int64_t t, int64_t last)
{
    return p.timeout_us > 0 && (last == INT64_MIN || (t >= p.timeout_us && last < t - p.timeout_us));
}

static int one(std::mt19937_64 &rng, int n, int K, const rm_nbtable_params &prm, bool with_pin, bool per_packet_rssi, bool with_sinr)
{
    const size_t nk = size_t(n) * size_t(K);
    const int n_pkt = int(rng() % 6);
    auto src = block<int32_t>(size_t(n_pkt));
    auto start = block<int64_t>(size_t(n_pkt));
    auto off = block<uint32_t>(size_t(n_pkt) + 1);
    off[0] = 0;
    for (int p = 0; p < n_pkt; ++p) {
        src[p] = rng() % 7 == 0 ? int32_t(n + rng() % 3) : rng() % 9 == 0 ? -1 : int32_t(rng() % uint64_t(n));
        start[p] = int64_t(rng() % 100000);
        off[p + 1] = off[p] + uint32_t(rng() % 3 == 0 ? 0 : rng() % uint64_t(n + 1));
    }
    const uint32_t L = off[n_pkt];
    auto dst = block<int32_t>(L);
    auto verdict = block<uint8_t>(L);
    auto rssi = block<double>(L), sinr = block<double>(L), pkt_rssi = block<double>(size_t(n_pkt));
    const double picks[8] = {-60.0, -60.0, -80.25, -95.0, -101.0, std::numeric_limits<double>::quiet_NaN(), INFINITY, -4e9};
    for (int p = 0; p < n_pkt; ++p) {
        pkt_rssi[p] = picks[rng() % 8];
        for (uint32_t i = off[p]; i < off[p + 1]; ++i) { // (ascending inside a packet; one junk receiver now and then)
            dst[i] = int32_t(i - off[p]);
            if (rng() % 13 == 0) dst[i] = n + 1;
            verdict[i] = rng() % 3 == 0 ? uint8_t(RM_INTERFERED) : uint8_t(RM_DELIVERED);
            rssi[i] = picks[rng() % 8];
            sinr[i] = double(int(rng() % 60)) - 10.5;
        }
    }
    rm_host_result r{};
    r.count = L;
    r.n_packets = uint32_t(n_pkt);
    r.pkt_offset = off.get();
    r.dst = dst.get();
    r.verdict = verdict.get();
    r.rssi = per_packet_rssi ? nullptr : rssi.get();
    r.pkt_rssi = per_packet_rssi ? pkt_rssi.get() : nullptr;
    r.sinr = with_sinr ? sinr.get() : nullptr;
    auto peer = block<int32_t>(nk), peer0 = block<int32_t>(nk), pin = block<int32_t>(size_t(n));
    auto st = block<rm_link_stats>(nk), st0 = block<rm_link_stats>(nk);
    for (int d = 0; d < n; ++d) {
        pin[d] = rng() % 4 == 0 ? -1 : rng() % 6 == 0 ? INT32_MIN : int32_t(rng() % uint64_t(n));
        for (int k = 0; k < K; ++k) {
            const size_t at = size_t(d) * K + k;
            const uint64_t pick = rng() % 12;
            int32_t v = pick == 0 ? -1 : pick == 1 ? n : pick == 2 ? INT32_MAX : pick == 3 ? d : int32_t(rng() % uint64_t(n));
            for (int m = 0; m < k; ++m)
                if (peer[size_t(d) * K + m] == v) v = -1; // (a row's valid entries are distinct)
            peer[at] = v;
            std::memset(&st[at], 0, sizeof(rm_link_stats));
            st[at].heard = rng() % 17 == 0 ? UINT64_MAX : rng() % 30;
            st[at].delivered = rng() % 5 == 0 ? 0 : rng() % (st[at].heard % 40 + 1);
            st[at].first_start_us = INT64_MAX;
            st[at].last_start_us = rng() % 4 == 0 ? INT64_MIN : rng() % 9 == 0 ? INT64_MAX : int64_t(rng() % 200000);
        }
    }
    std::memcpy(peer0.get(), peer.get(), nk * 4);
    std::memcpy(st0.get(), st.get(), nk * sizeof(rm_link_stats));
    auto node = block<rm_nbtable_node>(size_t(n));
    std::memset(node.get(), 0, size_t(n) * sizeof(rm_nbtable_node));
    rm_nbtable_totals tot{};
    const int64_t t = int64_t(rng() % 300000);
    const int32_t *pin_arg = with_pin ? pin.get() : nullptr;
    CHECK(rm_nbtable_from_result(&r, src.get(), start.get(), n, K, peer.get(), st.get(), &prm, t, pin_arg, node.get(), &tot) == RM_OK);
    CHECK(tot.updates == 1 && tot.skipped_slots == 0 && tot.expired == 0 && tot.reserved == 0);
    uint64_t adm = 0, es = 0, ep = 0, ref = 0;
    for (int d = 0; d < n; ++d) {
        const rm_nbtable_node &c = node[d];
        CHECK(c.admitted + c.refused <= 1 && c.admitted >= c.evicted_stale + c.evicted_poor && c.expired == 0);
        CHECK(c.reserved[0] == 0 && c.reserved[1] == 0 && c.reserved[2] == 0);
        adm += c.admitted; es += c.evicted_stale; ep += c.evicted_poor; ref += c.refused;
        int changed = 0, slot = -1;
        for (int k = 0; k < K; ++k) {
            const size_t at = size_t(d) * K + k;
            if (peer[at] != peer0[at]) {
                ++changed;
                slot = k;
                const bool pinned = with_pin && pin[d] >= 0 && pin[d] < n && peer0[at] == pin[d];
                CHECK(!held(n, d, peer0[at]) || !pinned);
            } else {
                CHECK(std::memcmp(&st[at], &st0[at], sizeof(rm_link_stats)) == 0); // (a slot whose peer stays keeps its entry)
            }
            for (int m = 0; m < k; ++m)
                CHECK(!held(n, d, peer[at]) || peer[size_t(d) * K + m] != peer[at]);
        }
        CHECK(changed == int(c.admitted));
        if (!c.admitted) continue;
        const int32_t s = peer[size_t(d) * K + slot];
        CHECK(held(n, d, s));
        uint64_t links = 0, deliv = 0;
        for (int p = 0; p < n_pkt; ++p)
            for (uint32_t i = off[p]; i < off[p + 1]; ++i)
                if (src[p] == s && dst[i] == d) {
                    ++links;
                    deliv += verdict[i] == uint8_t(RM_DELIVERED);
                }
        const rm_link_stats &e = st[size_t(d) * K + slot];
        CHECK(links >= 1 && e.heard == links && e.delivered == deliv && e.first_start_us <= e.last_start_us);
        if (!with_sinr) CHECK(e.sinr_q8_sum == 0);
    }
    CHECK(tot.admitted == adm && tot.evicted_stale == es && tot.evicted_poor == ep && tot.refused == ref);
    // the expire walk, on the tables as they are now
    std::memcpy(peer0.get(), peer.get(), nk * 4);
    std::memcpy(st0.get(), st.get(), nk * sizeof(rm_link_stats));
    const int64_t t2 = t + int64_t(rng() % 100000);
    CHECK(rm_nbtable_expire_tables(n, K, peer.get(), st.get(), &prm, t2, pin_arg, node.get(), &tot) == RM_OK);
    uint64_t expired = 0;
    for (int d = 0; d < n; ++d) {
        uint32_t mine = 0;
        for (int k = 0; k < K; ++k) {
            const size_t at = size_t(d) * K + k;
            const bool pinned = with_pin && pin[d] >= 0 && pin[d] < n && peer0[at] == pin[d];
            const bool goes = held(n, d, peer0[at]) && !pinned && stale(prm, t2, st0[at].last_start_us);
            mine += goes;
            if (goes) CHECK(peer[at] == -1 && st[at].heard == 0 && st[at].delivered == 0 && st[at].last_start_us == INT64_MIN && st[at].first_start_us == INT64_MAX);
            else CHECK(peer[at] == peer0[at] && std::memcmp(&st[at], &st0[at], sizeof(rm_link_stats)) == 0);
        }
        CHECK(node[d].expired == mine);
        expired += mine;
    }
    CHECK(tot.expired == expired && tot.updates == 1 && tot.admitted == adm);
    return 0;
}

int main()
{
    std::mt19937_64 rng(22);
    rm_nbtable_params base;
    rm_nbtable_defaults(&base);
    CHECK(base.admit_rssi_dbm == -95.0 && base.timeout_us == 60000000 && base.min_heard == 4 && base.evict_cost == 1024 && base.require_delivered == 1 &&
          base.reserved == 0);
    CHECK(rm_nbtable_validate(&base) == RM_OK && rm_nbtable_validate(nullptr) == RM_ERR_INVALID);
    rm_nbtable_defaults(nullptr);
    const int Ks[4] = {1, 2, 4, 8};
    for (int rep = 0; rep < 600; ++rep) {
        const int n = 1 + int(rng() % 24), K = Ks[rep % 4];
        rm_nbtable_params p = base;
        p.timeout_us = rep % 3 == 0 ? 0 : rep % 3 == 1 ? 50000 : int64_t(1) << 62;
        p.min_heard = rep % 5 == 0 ? 0u : rep % 5 == 1 ? 1u << 31 : 3u;
        p.evict_cost = rep % 7 == 0 ? 0u : rep % 7 == 1 ? UINT32_MAX : rep % 7 == 2 ? 128u : 400u;
        p.require_delivered = (rep / 2) % 2;
        if (one(rng, n, K, p, rep % 3 != 0, rep % 4 == 1, rep % 2 == 0)) return 1;
    }
    // empty inputs
    rm_host_result none{};
    rm_nbtable_totals t{};
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 0, 1, nullptr, nullptr, &base, 0, nullptr, nullptr, &t) == RM_OK && t.updates == 1);
    CHECK(rm_nbtable_expire_tables(0, 8, nullptr, nullptr, &base, 0, nullptr, nullptr, nullptr) == RM_OK);
    auto peer = block<int32_t>(2);
    auto st = block<rm_link_stats>(2);
    peer[0] = peer[1] = -1;
    std::memset(st.get(), 0, 2 * sizeof(rm_link_stats));
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), st.get(), &base, 5, nullptr, nullptr, nullptr) == RM_OK && peer[0] == -1);
    // refusals: nothing changes
    int32_t bad_pin[2] = {0, 2}, ok_pin[2] = {-5, 1};
    CHECK(rm_nbtable_from_result(nullptr, nullptr, nullptr, 2, 1, peer.get(), st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), st.get(), nullptr, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), st.get(), &base, -1, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, -1, 1, peer.get(), st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 3, peer.get(), st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, nullptr, st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), nullptr, &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), st.get(), &base, 0, bad_pin, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), st.get(), &base, 0, ok_pin, nullptr, nullptr) == RM_OK);
    rm_host_result some{};
    some.n_packets = 1;
    CHECK(rm_nbtable_from_result(&some, nullptr, nullptr, 2, 1, peer.get(), st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    some.count = 1;
    int32_t s1[1] = {0};
    int64_t b1[1] = {0};
    CHECK(rm_nbtable_from_result(&some, s1, b1, 2, 1, peer.get(), st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID); // (no columns)
    CHECK(rm_nbtable_expire_tables(2, 1, peer.get(), st.get(), nullptr, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_expire_tables(2, 1, peer.get(), st.get(), &base, -3, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_expire_tables(2, 16, peer.get(), st.get(), &base, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    CHECK(rm_nbtable_expire_tables(2, 1, peer.get(), st.get(), &base, 0, bad_pin, nullptr, nullptr) == RM_ERR_INVALID);
    for (int k = 0; k < 9; ++k) {
        rm_nbtable_params p = base;
        if (k == 0) p.admit_rssi_dbm = std::numeric_limits<double>::quiet_NaN();
        if (k == 1) p.admit_rssi_dbm = -INFINITY;
        if (k == 2) p.timeout_us = -1;
        if (k == 3) p.timeout_us = (int64_t(1) << 62) + 1;
        if (k == 4) p.min_heard = (1u << 31) + 1u;
        if (k == 5) p.evict_cost = 127;
        if (k == 6) p.require_delivered = 2;
        if (k == 7) p.require_delivered = -1;
        if (k == 8) p.reserved = 1;
        CHECK(rm_nbtable_validate(&p) == RM_ERR_INVALID);
        CHECK(rm_nbtable_from_result(&none, nullptr, nullptr, 2, 1, peer.get(), st.get(), &p, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
        CHECK(rm_nbtable_expire_tables(2, 1, peer.get(), st.get(), &p, 0, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
    }
    CHECK(peer[0] == -1 && peer[1] == -1 && st[0].heard == 0);
    std::printf("ok\n");
    return 0;
}
