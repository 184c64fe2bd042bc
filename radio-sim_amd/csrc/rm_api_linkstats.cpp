// rm_api_linkstats.cpp -- C ABI: watched-link statistics, per-link counters on the device (the pass is
// rm_linkstats.hip).
//
// The tables belong to the context, not to a medium or a tick slot: K peer slots and K rm_link_stats per node index and one
// rm_stats_totals.  The evaluating calls run the pass (through the seam of rm_api_passes.cpp); everything here enables, sets the
// peers, clears and reads.
#include "rm_host.hpp"

#include <algorithm>

using namespace rmh;

namespace rmh {

rm::LinkStatsDev linkstats_dev(const rm_context *c)
{
    rm::LinkStatsDev d{};
    d.peer = c->lk.peer.p;
    d.table = c->lk.table.p;
    d.totals = c->lk.totals.p;
    d.n_nodes = c->lk.n;
    d.K = c->lk.K;
    return d;
}

void linkstats_release(rm_context *c)
{
    rm_context::LinkStats &lk = c->lk;
    lk.peer.release(); lk.stage.release(); lk.table.release(); lk.totals.release(); lk.mark.release();
    lk.h.release();
    if (lk.h_bad) (void)hipHostFree(lk.h_bad);
    lk.h_bad = nullptr;
    lk.host_stale = false;
}

int linkstats_host_fresh(rm_context *c)
{
    rm_context::LinkStats &lk = c->lk;
    if (!lk.host_stale) return RM_OK;
    if (!lk.host.empty()) {
        RM_HIP(hipMemcpyAsync(lk.host.data(), lk.peer.p, lk.host.size() * 4, hipMemcpyDeviceToHost, c->stream));
        RM_HIP(hipStreamSynchronize(c->stream));
    }
    lk.host_stale = false;
    return RM_OK;
}

// off: nothing is launched afterwards, the tables released (pointers handed out end here)
static int linkstats_off(rm_context *c)
{
    rm_context::LinkStats &lk = c->lk;
    if (lk.n >= 0) RM_HIP(hipStreamSynchronize(c->stream)); // (a pass in flight still reads and adds to the tables)
    nbtable_release(c); // (the neighbour tables, E22, write these tables: they go off with them)
    lk.K = 0;
    lk.n = -1;
    lk.host.clear();
    lk.host.shrink_to_fit();
    linkstats_release(c);
    return RM_OK;
}

int linkstats_nodes_changed(rm_context *c)
{
    if (c->lk.n < 0 || c->lk.n == c->n) return RM_OK; // off, or the same node count: the tables stay
    return linkstats_off(c);
}

static size_t linkstats_entries(const rm_context *c) { return size_t(std::max(c->lk.n, 1)) * size_t(c->lk.K); }

int linkstats_have(const rm_context *c)
{
    if (!linkstats_on(c) || c->lk.n < 0) return fail(RM_ERR_STATE, "no watched-link statistics: rm_linkstats_enable(ctx, K) comes first");
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_linkstats_enable(rm_context *c, int32_t K)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (K != 0 && K != 1 && K != 2 && K != 4 && K != 8) return fail(RM_ERR_INVALID, "K is 1, 2, 4 or 8 (0: off)");
    RM_HIP(hipSetDevice(c->device));
    if (K == 0) return linkstats_off(c);
    RM_TRY(graphs_refuse(c, "the watched links' pass is not part of them"));
    rm_context::LinkStats &lk = c->lk;
    if (lk.K == K && lk.n == c->n) return RM_OK; // the same K again: nothing changes
    RM_TRY(linkstats_off(c));
    const size_t entries = size_t(std::max(c->n, 1)) * size_t(K);
    RM_HIP(lk.peer.ensure(entries));
    RM_HIP(lk.table.ensure(entries));
    RM_HIP(lk.totals.ensure(1));
    RM_HIP(rm::launch_linkstats_clear(c->stream, lk.peer.p, lk.table.p, entries));
    RM_HIP(hipMemsetAsync(lk.totals.p, 0, sizeof(rm_stats_totals), c->stream));
    lk.host.assign(size_t(c->n) * size_t(K), -1);
    lk.n = c->n;
    lk.K = K;
    return RM_OK;
}

int rm_linkstats_enabled(const rm_context *c) { return c ? c->lk.K : 0; }

int rm_linkstats_watch(rm_context *c, const int32_t *nodes, int32_t n, const int32_t *peers)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(linkstats_have(c));
    rm_context::LinkStats &lk = c->lk;
    // the whole list is validated before anything changes
    RM_TRY(rm_linkstats_validate(lk.n, lk.K, nodes, n, peers));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    if (nodes) RM_TRY(linkstats_host_fresh(c)); // (a list updates rows of the host's copy; the whole table replaces it)
    else lk.host_stale = false;
    const size_t K = size_t(lk.K);
    if (!nodes) {
        // the whole table: staged in device memory from the host's copy, and waited for -- a later update of the copy cannot race
        std::memcpy(lk.host.data(), peers, size_t(n) * K * 4);
        RM_HIP(lk.stage.ensure(size_t(n) * K));
        RM_HIP(hipMemcpyAsync(lk.stage.p, lk.host.data(), size_t(n) * K * 4, hipMemcpyHostToDevice, c->stream));
        RM_HIP(rm::launch_linkstats_scatter(c->stream, lk.peer.p, lk.table.p, lk.n, lk.K, nullptr, n, lk.stage.p));
        RM_HIP(hipStreamSynchronize(c->stream));
        return RM_OK;
    }
    // a list: the peer rows and the list staged in the block (rows of K * 4 bytes), one launch of the watch rule, not waited for
    RM_TRY(lk.h.ensure(c->stream, size_t(n), K * 4));
    std::memcpy(lk.h.rows(), peers, size_t(n) * K * 4);
    std::memcpy(lk.h.nodes(), nodes, size_t(n) * 4);
    for (int32_t r = 0; r < n; ++r) std::memcpy(lk.host.data() + size_t(nodes[r]) * K, peers + size_t(r) * K, K * 4);
    RM_HIP(rm::launch_linkstats_scatter(c->stream, lk.peer.p, lk.table.p, lk.n, lk.K, lk.h.nodes(), n, reinterpret_cast<const int32_t *>(lk.h.rows())));
    return RM_OK;
}

int rm_linkstats_peers_get(rm_context *c, const int32_t *nodes, int32_t n, int32_t *out)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(linkstats_have(c));
    const rm_context::LinkStats &lk = c->lk;
    RM_TRY(check_node_list(nodes, n, lk.n));
    if (lk.host_stale) {
        RM_HIP(hipSetDevice(c->device));
        RM_TRY(linkstats_host_fresh(c));
    }
    const size_t K = size_t(lk.K);
    for (int32_t r = 0; r < n; ++r) std::memcpy(out + size_t(r) * K, lk.host.data() + size_t(nodes ? nodes[r] : r) * K, K * 4);
    return RM_OK;
}

int rm_linkstats_read(rm_context *c, const int32_t *nodes, int32_t n, rm_link_stats *out, rm_stats_totals *totals)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(linkstats_have(c));
    rm_context::LinkStats &lk = c->lk;
    RM_TRY(check_node_list(nodes, n, lk.n));
    RM_HIP(hipSetDevice(c->device));
    return rows_read(c, lk.h, lk.table.p, lk.K * int(sizeof(rm_link_stats) / 8), lk.n, nodes, n, out, lk.totals.p, totals);
}

int rm_linkstats_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(linkstats_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(rm::launch_linkstats_clear(c->stream, nullptr, c->lk.table.p, linkstats_entries(c)));
    RM_HIP(hipMemsetAsync(c->lk.totals.p, 0, sizeof(rm_stats_totals), c->stream));
    return RM_OK;
}

int rm_linkstats_device(rm_context *c, const int32_t **dev_peer, const rm_link_stats **dev_table, const rm_stats_totals **dev_totals)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(linkstats_have(c));
    if (dev_peer) *dev_peer = c->lk.peer.p;
    if (dev_table) *dev_table = c->lk.table.p;
    if (dev_totals) *dev_totals = c->lk.totals.p;
    return RM_OK;
}

int64_t rm_linkstats_q8(double x) { return rm::host_linkstats_q8(x); }

int rm_linkstats_validate(int32_t n_nodes, int32_t K, const int32_t *nodes, int32_t n, const int32_t *peers)
{
    if (K != 1 && K != 2 && K != 4 && K != 8) return fail(RM_ERR_INVALID, "K is 1, 2, 4 or 8");
    if (n_nodes < 0 || n < 0 || (n > 0 && !peers)) return fail(RM_ERR_INVALID, "bad arguments");
    if (!nodes) RM_TRY(check_node_list(nullptr, n, n_nodes)); // (the count alone: a listed node is checked with its row, below)
    for (int32_t r = 0; r < n; ++r) {
        const int32_t node = nodes ? nodes[r] : r;
        if (node < 0 || node >= n_nodes) return fail(RM_ERR_INVALID, "node index out of range");
        const int32_t *row = peers + size_t(r) * size_t(K);
        for (int32_t k = 0; k < K; ++k) {
            const int32_t p = row[k];
            if (p == -1) continue;
            if (p < 0 || p >= n_nodes) return fail(RM_ERR_INVALID, "a peer is -1 or a node index");
            if (p == node) return fail(RM_ERR_INVALID, "a node does not watch itself");
            for (int32_t m = 0; m < k; ++m)
                if (row[m] == p) return fail(RM_ERR_INVALID, "the peers of a row are distinct");
        }
    }
    if (nodes && n > 1) { // a node appears at most once
        std::vector<int32_t> sorted(nodes, nodes + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(RM_ERR_INVALID, "a node appears at most once in the list");
    }
    return RM_OK;
}

} // extern "C"
