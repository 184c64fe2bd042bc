// linkest_host_san_test.cpp -- rm_linkest_fold_tables, rm_linkest_validate and rm_linkest_defaults
// (radio-sim_amd/csrc/rm_api_linkest.cpp), the pure host forms of the link estimator (extension E23), under AddressSanitizer +
// UndefinedBehaviorSanitizer: host code only, no device is touched.  tests/test_linkest_ref.py compiles rm_api_linkest.cpp beside
// this file with -fsanitize=address,undefined and runs it.  Every array is a heap block of exactly the size the call may touch, so
// a write or a read one element beyond is reported.
// Checks, over sequences of folds on random tables (junk peers, duplicate peers, counters that shrink, counters near 2^40 and near
// 2^64, junk next hops): every estimate is 0 or within 128 .. max_etx; the published table equals what the entries say; an entry's
// peer is -1 or the input slot's peer; the per-node counters add up to the totals and estimates is the number of entries with an
// estimate; the inputs are not written; the measured-route query's entry cost of a published entry is its etx; empty inputs; every
// refusal.  Prints "ok".
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

template <typename T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(n > 0 ? new T[n]() : nullptr); }

static int one(std::mt19937_64 &rng, int n, int K, const rm_linkest_params &prm, bool with_fwd)
{
    const size_t nk = size_t(n) * size_t(K);
    auto peer = block<int32_t>(nk), pub_peer = block<int32_t>(nk), peer_copy = block<int32_t>(nk);
    auto stats = block<rm_link_stats>(nk), pub_stats = block<rm_link_stats>(nk), stats_copy = block<rm_link_stats>(nk);
    auto fwd = block<rm_fwd_node>(size_t(n)), fwd_copy = block<rm_fwd_node>(size_t(n));
    auto entry = block<rm_linkest_entry>(nk);
    auto node = block<rm_linkest_node>(size_t(n));
    rm_linkest_totals tot{};
    for (size_t i = 0; i < nk; ++i) {
        entry[i].peer = -1;
        pub_peer[i] = -1;
        pub_stats[i].first_start_us = INT64_MAX;
        pub_stats[i].last_start_us = INT64_MIN;
        peer[i] = rng() % 5 == 0 ? int32_t(rng() % 7) - 3 + (rng() % 2 ? n : 0) : int32_t(rng() % uint64_t(n));
        stats[i].heard = rng() % 7 == 0 ? (1ull << 40) - rng() % 50 : rng() % 11 == 0 ? ~0ull - rng() % 50 : 0;
        stats[i].delivered = stats[i].heard / (1 + rng() % 3);
    }
    for (int j = 0; j < n; ++j) {
        node[j].base_next = -1;
        fwd[j].next = int32_t(rng() % uint64_t(n + 3)) - 2;
    }
    const rm_linkest_inputs in{peer.get(), stats.get(), with_fwd ? fwd.get() : nullptr, K, 0};
    for (int fold = 0; fold < 12; ++fold) {
        for (size_t i = 0; i < nk; ++i) {
            const uint64_t dh = rng() % 5;
            stats[i].heard += dh;                             // (unsigned: wraps near 2^64, which the rule sees as a shrink)
            stats[i].delivered += dh ? rng() % (dh + 2) : 0;  // (now and then delivered > heard)
            if (rng() % 40 == 0) peer[i] = int32_t(rng() % uint64_t(n + 2)) - 1;
            if (rng() % 40 == 0) stats[i].heard = stats[i].delivered = 0;
            if (K > 1 && rng() % 40 == 0) peer[i] = peer[i - i % size_t(K)];
        }
        for (int j = 0; j < n; ++j) {
            fwd[j].acked += rng() % 4;
            fwd[j].failed += rng() % 3;
            if (rng() % 20 == 0) fwd[j].next = int32_t(rng() % uint64_t(n + 3)) - 2;
            if (rng() % 20 == 0) fwd[j].acked = fwd[j].failed = 0;
        }
        if (nk) std::memcpy(peer_copy.get(), peer.get(), nk * sizeof(int32_t));
        if (nk) std::memcpy(static_cast<void *>(stats_copy.get()), stats.get(), nk * sizeof(rm_link_stats));
        if (n) std::memcpy(static_cast<void *>(fwd_copy.get()), fwd.get(), size_t(n) * sizeof(rm_fwd_node));
        CHECK(rm_linkest_fold_tables(n, &in, &prm, entry.get(), node.get(), pub_peer.get(), pub_stats.get(), &tot) == RM_OK);
        CHECK(!nk || std::memcmp(peer_copy.get(), peer.get(), nk * sizeof(int32_t)) == 0);
        CHECK(!nk || std::memcmp(stats_copy.get(), stats.get(), nk * sizeof(rm_link_stats)) == 0);
        CHECK(!n || std::memcmp(fwd_copy.get(), fwd.get(), size_t(n) * sizeof(rm_fwd_node)) == 0);
        uint64_t estimates = 0, restarted = 0, samples = 0, unmatched = 0;
        rm_etx_params ep;
        rm_etx_defaults(&ep);
        ep.min_heard = 1;
        ep.max_link_cost = 65535;
        for (size_t i = 0; i < nk; ++i) {
            const int j = int(i / size_t(K));
            const rm_linkest_entry &e = entry[i];
            const bool empty = peer[i] < 0 || peer[i] >= n || peer[i] == j;
            CHECK(e.peer == (empty ? -1 : peer[i]));
            CHECK(e.etx == 0 || (e.etx >= 128 && e.etx <= prm.max_etx));
            CHECK(e.peer != -1 || (e.etx == 0 && e.windows == 0 && e.data_windows == 0 && e.base_heard == 0 && e.base_delivered == 0));
            CHECK((e.etx != 0) == (e.windows + e.data_windows != 0)); // (a sample is at least 128)
            CHECK(pub_peer[i] == e.peer);
            const rm_link_stats &s = pub_stats[i];
            CHECK(s.heard == e.etx && s.delivered == (e.etx ? 128u : 0u) && s.rssi_q8_sum == 0 && s.sinr_q8_sum == 0);
            CHECK(s.first_start_us == INT64_MAX && s.last_start_us == INT64_MIN);
            uint32_t cost = 0;
            CHECK(rm_etx_link_cost(&ep, s.heard, s.delivered, &cost) == (e.etx ? 1 : 0) && cost == e.etx);
            estimates += e.etx != 0;
        }
        for (int j = 0; j < n; ++j) {
            restarted += node[j].restarted;
            samples += node[j].data_samples;
            unmatched += node[j].data_unmatched;
            CHECK(with_fwd && prm.data_window ? node[j].base_next == fwd[j].next : node[j].base_next == -1);
        }
        CHECK(tot.folds == uint64_t(fold) + 1 && tot.estimates == estimates && tot.restarted == restarted && tot.data_samples == samples);
        CHECK(tot.data_unmatched == unmatched && tot.reserved == 0);
        CHECK(with_fwd || (samples == 0 && unmatched == 0));
        CHECK(prm.beacon_window != 0 || tot.beacon_samples == 0);
    }
    return 0;
}

int main()
{
    rm_linkest_params d;
    rm_linkest_defaults(&d);
    CHECK(d.beacon_window == 3 && d.data_window == 5 && d.beacon_alpha_q8 == 230 && d.data_alpha_q8 == 230 && d.max_etx == 6400 && d.reserved == 0);
    CHECK(rm_linkest_validate(&d) == RM_OK && rm_linkest_validate(nullptr) == RM_ERR_INVALID);
    rm_linkest_defaults(nullptr);
    std::mt19937_64 rng(23);
    const int Ks[4] = {1, 2, 4, 8};
    for (int round = 0; round < 60; ++round) {
        rm_linkest_params p = d;
        p.beacon_window = uint32_t(rng() % 5);
        p.data_window = uint32_t(rng() % 7);
        p.beacon_alpha_q8 = uint32_t(rng() % 256);
        p.data_alpha_q8 = uint32_t(rng() % 256);
        p.max_etx = round % 7 == 0 ? 128u : round % 5 == 0 ? 65535u : 128u + uint32_t(rng() % 9000);
        if (one(rng, 1 + int(rng() % 20), Ks[round % 4], p, round % 3 != 0)) return 1; // (a NULL table is refused: n >= 1)
    }
    // refusals: nothing is touched
    int32_t peer[2] = {1, 0}, pub[2] = {-1, -1};
    rm_link_stats st[2] = {}, ps[2] = {};
    rm_linkest_entry e[2] = {};
    rm_linkest_node nd[2] = {};
    rm_linkest_totals tot{};
    e[0].peer = e[1].peer = -1; // (the after-enable state)
    nd[0].base_next = nd[1].base_next = -1;
    rm_linkest_inputs in{peer, st, nullptr, 1, 0};
    CHECK(rm_linkest_fold_tables(2, nullptr, &d, e, nd, pub, ps, &tot) == RM_ERR_INVALID);
    CHECK(rm_linkest_fold_tables(2, &in, nullptr, e, nd, pub, ps, &tot) == RM_ERR_INVALID);
    CHECK(rm_linkest_fold_tables(-1, &in, &d, e, nd, pub, ps, &tot) == RM_ERR_INVALID);
    CHECK(rm_linkest_fold_tables(2, &in, &d, nullptr, nd, pub, ps, &tot) == RM_ERR_INVALID);
    CHECK(rm_linkest_fold_tables(2, &in, &d, e, nullptr, pub, ps, &tot) == RM_ERR_INVALID);
    CHECK(rm_linkest_fold_tables(2, &in, &d, e, nd, nullptr, ps, &tot) == RM_ERR_INVALID);
    CHECK(rm_linkest_fold_tables(2, &in, &d, e, nd, pub, nullptr, &tot) == RM_ERR_INVALID);
    for (int bad = 0; bad < 4; ++bad) {
        rm_linkest_inputs b = in;
        if (bad == 0) b.K = 3;
        if (bad == 1) b.reserved = 1;
        if (bad == 2) b.peer = nullptr;
        if (bad == 3) b.stats = nullptr;
        CHECK(rm_linkest_fold_tables(2, &b, &d, e, nd, pub, ps, &tot) == RM_ERR_INVALID);
    }
    for (int bad = 0; bad < 6; ++bad) {
        rm_linkest_params p = d;
        if (bad == 0) p.beacon_window = (1u << 31) + 1u;
        if (bad == 1) p.data_window = (1u << 31) + 1u;
        if (bad == 2) p.beacon_alpha_q8 = 256;
        if (bad == 3) p.data_alpha_q8 = 256;
        if (bad == 4) p.max_etx = bad % 2 ? 65536u : 127u;
        if (bad == 5) p.reserved = 1;
        CHECK(rm_linkest_validate(&p) == RM_ERR_INVALID && rm_linkest_fold_tables(2, &in, &p, e, nd, pub, ps, &tot) == RM_ERR_INVALID);
    }
    CHECK(tot.folds == 0 && pub[0] == -1 && e[0].etx == 0);
    CHECK(rm_linkest_fold_tables(2, &in, &d, e, nd, pub, ps, nullptr) == RM_OK && pub[0] == 1 && pub[1] == 0); // (totals may be NULL)
    CHECK(rm_linkest_fold_tables(0, &in, &d, nullptr, nullptr, nullptr, nullptr, &tot) == RM_OK && tot.folds == 1);
    std::printf("ok\n");
    return 0;
}
