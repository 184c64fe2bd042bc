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
    rm_context::Stats &st = c->st;
    RM_TRY(check_node_list(nodes, n, st.n));
    RM_HIP(hipSetDevice(c->device));
    return rows_read(c, st.h, st.table.p, sizeof(rm_node_stats) / 8, st.n, nodes, n, out, st.totals.p, totals);
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
