// rm_api_stats.cpp -- C ABI: per-node traffic counters accumulated on the device (the pass is rm_stats.hip).
//
// The table belongs to the context, not to a medium or a tick slot: one rm_node_stats per node index and one rm_stats_totals.
// The evaluating calls add to it (through the seam of rm_api_passes.cpp); everything here enables, zeroes and reads it.
#include "rm_host.hpp"

using namespace rmh;

namespace rmh {

rm::StatsDev stats_dev(const rm_context *c)
{
    rm::StatsDev d{};
    d.table = c->st.table.p;
    d.totals = c->st.totals.p;
    d.n_nodes = c->st.n;
    return d;
}

// the table for c->n nodes, zeroed (with the totals) when it is new or the node count is another one
static int stats_size(rm_context *c)
{
    rm_context::Stats &st = c->st;
    if (st.n == c->n && st.table.p && st.totals.p) return RM_OK;
    RM_HIP(hipStreamSynchronize(c->stream)); // (a pass in flight may still add to the table about to be replaced)
    RM_HIP(st.table.ensure(size_t(std::max(c->n, 1))));
    RM_HIP(st.totals.ensure(1));
    RM_HIP(hipMemsetAsync(st.table.p, 0, st.table.n * sizeof(rm_node_stats), c->stream));
    RM_HIP(hipMemsetAsync(st.totals.p, 0, sizeof(rm_stats_totals), c->stream));
    st.n = c->n;
    return RM_OK;
}

int stats_nodes_changed(rm_context *c)
{
    if (c->st.n < 0 || c->st.n == c->n) return RM_OK; // never enabled, or the same node count: the counters stay
    return stats_size(c);
}

// the pinned, host-mapped block of a list read: records out, then the totals, then the list in.  (The block waits for the stream
// whether it grows or not; the one caller waits for it again behind its launch, so the wait here finds little left to wait for)
static int stats_host_block(rm_context *c, int32_t n, rm_node_stats **h_out, rm_stats_totals **h_totals, int32_t **h_nodes)
{
    PinnedBlock &h = c->st.h;
    RM_TRY(h.ensure(c->stream, size_t(n), [](size_t cap) { return cap * sizeof(rm_node_stats) + pad64(sizeof(rm_stats_totals)) + pad64(cap * 4); }));
    *h_out = reinterpret_cast<rm_node_stats *>(h.p);
    *h_totals = reinterpret_cast<rm_stats_totals *>(h.p + h.cap * sizeof(rm_node_stats));
    *h_nodes = reinterpret_cast<int32_t *>(h.p + h.cap * sizeof(rm_node_stats) + pad64(sizeof(rm_stats_totals)));
    return RM_OK;
}

static int stats_have(const rm_context *c)
{
    if (c->st.n < 0) return fail(RM_ERR_STATE, "no statistics: rm_stats_enable(ctx, 1) comes first");
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_stats_enable(rm_context *c, int32_t on)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (!on) {
        c->st.on = false;
        return RM_OK;
    }
    RM_TRY(graphs_refuse(c, "the counters' pass is not part of them"));
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(stats_size(c));
    c->st.on = true;
    return RM_OK;
}

int rm_stats_enabled(const rm_context *c) { return (c && c->st.on) ? 1 : 0; }

int rm_stats_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(stats_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(hipMemsetAsync(c->st.table.p, 0, c->st.table.n * sizeof(rm_node_stats), c->stream));
    RM_HIP(hipMemsetAsync(c->st.totals.p, 0, sizeof(rm_stats_totals), c->stream));
    return RM_OK;
}

int rm_stats_read(rm_context *c, const int32_t *nodes, int32_t n, rm_node_stats *out, rm_stats_totals *totals)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(stats_have(c));
    const rm_context::Stats &st = c->st;
    RM_TRY(check_node_list(nodes, n, st.n));
    RM_HIP(hipSetDevice(c->device));
    if (!nodes || n == 0) { // the whole table in node order (or the totals alone): copies on the stream, one synchronisation
        if (n > 0) RM_HIP(hipMemcpyAsync(out, st.table.p, size_t(n) * sizeof(rm_node_stats), hipMemcpyDeviceToHost, c->stream));
        if (totals) RM_HIP(hipMemcpyAsync(totals, st.totals.p, sizeof(rm_stats_totals), hipMemcpyDeviceToHost, c->stream));
        RM_HIP(hipStreamSynchronize(c->stream));
        return RM_OK;
    }
    // a list: one small gather launch reads it from the host-mapped block and writes the records and the totals there
    rm_node_stats *h_out;
    rm_stats_totals *h_totals;
    int32_t *h_nodes;
    RM_TRY(stats_host_block(c, n, &h_out, &h_totals, &h_nodes));
    std::memcpy(h_nodes, nodes, size_t(n) * 4);
    RM_HIP(rm::launch_stats_gather(c->stream, stats_dev(c), h_nodes, n, h_out, h_totals));
    RM_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(out, h_out, size_t(n) * sizeof(rm_node_stats));
    if (totals) *totals = *h_totals;
    return RM_OK;
}

int rm_stats_device(rm_context *c, const rm_node_stats **dev_table, const rm_stats_totals **dev_totals)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(stats_have(c));
    if (dev_table) *dev_table = c->st.table.p;
    if (dev_totals) *dev_totals = c->st.totals.p;
    return RM_OK;
}

} // extern "C"
