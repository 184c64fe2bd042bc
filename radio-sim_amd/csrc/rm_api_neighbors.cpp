// rm_api_neighbors.cpp -- C ABI: the neighbour query, each node's K strongest potential links on the device (DESIGN.md section 6,
// E16; the kernels are rm_neighbors.hip), and rm_linkstats_watch_device, which takes such rows into the watched-link statistics
// without the host seeing them.
//
// The query READS the node table and the model and writes the caller's outputs and two scratch blocks of its own
// (rm_context::Neighbors): no tick slot, no result buffer, no on-air window, not the generator, none of E11-E15's tables, not the
// source-candidate cache.  An evaluating call after a query gives what it gave without one.
#include "rm_query.hpp"

using namespace rmh;

namespace rmh {

void neighbors_release(rm_context *c)
{
    c->nb.prep.release();
    c->nb.off_list.release();
}

// what both forms refuse, before anything is launched
static int neighbors_check(rm_context *c, int32_t direction, int32_t K, bool have_list, int32_t n, const void *peer)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (direction != RM_NB_HEARD_BY && direction != RM_NB_HEARS) return fail(RM_ERR_INVALID, "direction is RM_NB_HEARD_BY or RM_NB_HEARS");
    if (K < 1 || K > RM_NB_MAX_K) return fail(RM_ERR_INVALID, "K outside 1 .. RM_NB_MAX_K");
    if (n < 0) return fail(RM_ERR_INVALID, "negative entry count");
    if (!peer) return fail(RM_ERR_INVALID, "peer is NULL");
    if (!have_list) RM_TRY(check_node_list(nullptr, n, c->n)); // (the count; the host form checks its list once this has passed)
    if (c->params.kind != RM_MODEL_LOGDIST)
        return fail(RM_ERR_STATE, "the neighbour query ranks links by rssi: only the log-distance medium computes one per link");
    if (c->in_tick) return fail(RM_ERR_STATE, "rm_neighbors_query between rm_tick_begin and rm_tick_flush");
    if (part_count(c) != c->n || part_spatial(c))
        return fail(RM_ERR_STATE, "the neighbour query needs the whole receiver table: this context has a receiver partition");
    RM_TRY(graphs_refuse(c, "the neighbour query is not part of them"));
    if (int64_t(n) * int64_t(K) > (int64_t(1) << 27)) return fail(RM_ERR_CAPACITY, "n * K above 2^27");
    return RM_OK;
}

// the launches on the context's stream; list / peer / rssi / degree are device-visible memory
static int neighbors_launch(rm_context *c, int32_t direction, int32_t K, const int32_t *list, int32_t n, int32_t *peer, double *rssi, int32_t *degree)
{
    RM_TRY(prepare_nodes(c)); // pending node changes first, as a tick does
    if (c->n_rx != c->n) return fail(RM_ERR_STATE, "internal: the receiver table does not hold every node");
    rm::NbDev q{};
    q.list = list;
    q.n = n;
    q.K = K;
    q.peer = peer;
    q.rssi = reinterpret_cast<uint64_t *>(rssi);
    q.degree = degree;
    if (direction == RM_NB_HEARS) {
        rm_context::Neighbors &nb = c->nb;
        RM_TRY(grow(c, need(nb.prep, 2), need(nb.off_list, size_t(std::max(c->n, 1)))));
        RM_HIP(hipMemsetAsync(nb.prep.p, 0, 2 * sizeof(unsigned long long), c->stream));
        q.prep = nb.prep.p;
        q.off_list = nb.off_list.p;
    }
    CallProbe probe(c); // (rm_profile_kernels names the path that ran)
    RM_HIP(rm::launch_nb_query(c->stream, nodes_dev(c), model_dev(c), q, direction, nb_needs_scan(c)));
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_neighbors_query_device(rm_context *c, int32_t direction, int32_t K, const int32_t *dev_nodes, int32_t n, int32_t *dev_peer,
                              double *dev_rssi, int32_t *dev_degree)
{
    RM_TRY(neighbors_check(c, direction, K, dev_nodes != nullptr, n, dev_peer));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    return neighbors_launch(c, direction, K, dev_nodes, n, dev_peer, dev_rssi, dev_degree);
}

int rm_neighbors_query(rm_context *c, int32_t direction, int32_t K, const int32_t *nodes, int32_t n, int32_t *peer, double *rssi, int32_t *degree)
{
    RM_TRY(neighbors_check(c, direction, K, nodes != nullptr, n, peer));
    RM_TRY(check_node_list(nodes, n, c->n));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    // the call's device block lives for this call only: list, rows, rssi, degrees
    const size_t rows = size_t(n) * size_t(K);
    CallBlock b(c);
    const size_t o_nodes = b.reserve(size_t(n) * 4), o_rssi = b.reserve(rows * 8), o_peer = b.reserve(rows * 4), o_deg = b.reserve(size_t(n) * 4);
    RM_TRY(b.alloc());
    int32_t *d_nodes = b.at<int32_t>(o_nodes, nodes), *d_peer = b.at<int32_t>(o_peer), *d_deg = b.at<int32_t>(o_deg, degree);
    double *d_rssi = b.at<double>(o_rssi, rssi);
    b.in(d_nodes, nodes, size_t(n) * 4);
    const int rc = b.ok() ? neighbors_launch(c, direction, K, d_nodes, n, d_peer, d_rssi, d_deg) : RM_OK;
    if (rc == RM_OK) {
        b.out(peer, d_peer, rows * 4);
        b.out(rssi, d_rssi, rows * 8);
        b.out(degree, d_deg, size_t(n) * 4);
    }
    return b.finish(rc, "rm_neighbors_query");
}

int rm_neighbors_from_result(const rm_host_result *r, int32_t n_pkt, int32_t K, int32_t *peer, double *rssi, int32_t *degree)
{
    if (!r || !peer) return fail(RM_ERR_INVALID, "r or peer is NULL");
    if (K < 1 || K > RM_NB_MAX_K) return fail(RM_ERR_INVALID, "K outside 1 .. RM_NB_MAX_K");
    if (n_pkt < 0 || uint32_t(n_pkt) > r->n_packets) return fail(RM_ERR_INVALID, "n_pkt outside 0 .. the result's packets");
    const bool have = r->pkt_offset && r->dst && (r->rssi || r->pkt_rssi);
    if (n_pkt > 0 && r->count > 0 && !have) return fail(RM_ERR_INVALID, "the result lacks pkt_offset, dst or an rssi column");
    const double nan = quiet_nan();
    for (int32_t p = 0; p < n_pkt; ++p) {
        int32_t top_n[RM_NB_MAX_K];
        double top_r[RM_NB_MAX_K];
        int32_t cnt = 0, deg = 0;
        if (have) {
            const uint32_t end = std::min(r->pkt_offset[p + 1], r->count);
            const uint32_t first = std::min(r->pkt_offset[p], end);
            for (uint32_t i = first; i < end; ++i) {
                const double v = r->rssi ? r->rssi[i] : r->pkt_rssi[p];
                const int32_t node = r->dst[i];
                if (v != v) continue; // (a NaN rssi is no link)
                ++deg;
                // insertion by the rule: rssi descending, then node index ascending
                int32_t at = cnt;
                while (at > 0 && (v > top_r[at - 1] || (v == top_r[at - 1] && node < top_n[at - 1]))) --at;
                if (at >= K) continue;
                const int32_t last = std::min(cnt, K - 1);
                for (int32_t k = last; k > at; --k) {
                    top_r[k] = top_r[k - 1];
                    top_n[k] = top_n[k - 1];
                }
                top_r[at] = v;
                top_n[at] = node;
                cnt = std::min(cnt + 1, K);
            }
        }
        for (int32_t k = 0; k < K; ++k) {
            peer[size_t(p) * size_t(K) + size_t(k)] = k < cnt ? top_n[k] : -1;
            if (rssi) rssi[size_t(p) * size_t(K) + size_t(k)] = k < cnt ? top_r[k] : nan;
        }
        if (degree) degree[p] = deg;
    }
    return RM_OK;
}

int rm_linkstats_stage_device(rm_context *c, int32_t **dev_rows)
{
    if (!c || !dev_rows) return fail(RM_ERR_INVALID, "ctx or dev_rows is NULL");
    RM_TRY(linkstats_have(c));
    rm_context::LinkStats &lk = c->lk;
    RM_HIP(hipSetDevice(c->device));
    const size_t want = size_t(std::max(lk.n, 1)) * size_t(lk.K);
    if (lk.stage.n < want) {
        RM_HIP(hipStreamSynchronize(c->stream)); // (an earlier launch may still read the old block)
        RM_HIP(lk.stage.ensure(want));
    }
    *dev_rows = lk.stage.p;
    return RM_OK;
}

int rm_linkstats_watch_device(rm_context *c, const int32_t *dev_nodes, int32_t n, const int32_t *dev_peers)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(linkstats_have(c));
    rm_context::LinkStats &lk = c->lk;
    if (n < 0 || (n > 0 && !dev_peers)) return fail(RM_ERR_INVALID, "bad arguments");
    if (!dev_nodes) RM_TRY(check_node_list(nullptr, n, lk.n)); // (the count; a list in device memory is checked on the device)
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    if (!lk.h_bad) RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&lk.h_bad), 64, hipHostMallocMapped));
    if (dev_nodes && lk.mark.n < size_t(std::max(lk.n, 1))) { // (a fresh array knows no stamp)
        RM_HIP(hipStreamSynchronize(c->stream));
        RM_HIP(lk.mark.ensure(size_t(std::max(lk.n, 1))));
        RM_HIP(hipMemsetAsync(lk.mark.p, 0, lk.mark.n * sizeof(uint32_t), c->stream));
        lk.stamp = 0;
    }
    if (dev_nodes && ++lk.stamp == 0u) { // (the stamps have gone round: forget the old ones)
        lk.stamp = 1u;
        RM_HIP(hipMemsetAsync(lk.mark.p, 0, lk.mark.n * sizeof(uint32_t), c->stream));
    }
    RM_HIP(hipStreamSynchronize(c->stream)); // (the flag word is the host's to write now)
    *lk.h_bad = 0u;
    {
        CallProbe probe(c);
        RM_HIP(rm::launch_nb_watch_check(c->stream, dev_nodes, n, dev_peers, lk.n, lk.K, lk.mark.p, lk.stamp, lk.h_bad));
    }
    RM_HIP(hipStreamSynchronize(c->stream));
    if (*lk.h_bad != 0u)
        return fail(RM_ERR_INVALID, "a row breaks the rules of rm_linkstats_watch: a node outside the table or listed twice, a peer that is "
                                    "neither -1 nor another node's index, or a peer twice in its row");
    // the existing watch rule: a slot whose peer changes is written and its entry cleared, the others keep their history
    RM_HIP(rm::launch_linkstats_scatter(c->stream, lk.peer.p, lk.table.p, lk.n, lk.K, dev_nodes, n, dev_peers));
    lk.host_stale = true;
    return RM_OK;
}

} // extern "C"
