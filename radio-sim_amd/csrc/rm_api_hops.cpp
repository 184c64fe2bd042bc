// rm_api_hops.cpp -- C ABI: the hop query, hop count and best parent toward a set of roots over the potential-link graph
// (the kernels are rm_hops.hip), the gather rm_hops_next_device, and the pure host form
// rm_hops_from_links.
//
// The query READS the node table and the model and writes the caller's outputs and scratch of its own (rm_context::Hops): no
// tick slot, no result buffer, no on-air window, not the generator, none of E11-E15's tables, not the source-candidate cache, not
// the neighbour query's scratch.  An evaluating call after a query gives what it gave without one.
#include "rm_query.hpp"

using namespace rmh;

namespace rmh {

void hops_release(rm_context *c)
{
    c->hp.words.release();
    c->hp.off_list.release();
    c->hp.queue.release();
    c->hp.h.release();
}

// what both forms refuse, before anything is launched
static int hops_check(rm_context *c, int32_t direction, double min_rssi, const int32_t *roots, int32_t n_roots, const rm_hops_out *out)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (!out || !out->hop) return fail(RM_ERR_INVALID, "out or out->hop is NULL");
    if (direction != RM_NB_HEARD_BY && direction != RM_NB_HEARS) return fail(RM_ERR_INVALID, "direction is RM_NB_HEARD_BY or RM_NB_HEARS");
    if (min_rssi != min_rssi) return fail(RM_ERR_INVALID, "min_rssi_dbm is NaN");
    RM_TRY(roots_check(roots, n_roots));
    if (c->params.kind != RM_MODEL_LOGDIST)
        return fail(RM_ERR_STATE, "the hop query walks links that have an rssi: only the log-distance medium computes one per link");
    if (c->in_tick) return fail(RM_ERR_STATE, "rm_hops_query between rm_tick_begin and rm_tick_flush");
    if (part_count(c) != c->n || part_spatial(c))
        return fail(RM_ERR_STATE, "the hop query needs the whole receiver table: this context has a receiver partition");
    RM_TRY(graphs_refuse(c, "the hop query is not part of them"));
    return RM_OK;
}

// the whole query on the context's stream; roots and the arrays of `out` are device-visible memory.  Returns with the stream idle.
static int hops_run(rm_context *c, int32_t direction, double min_rssi, const int32_t *roots, int32_t n_roots, const rm_hops_out &out,
                    rm_hops_totals *totals)
{
    rm_hops_totals t{0, -1, 0, 0};
    if (c->n > 0) {
        RM_TRY(prepare_nodes(c)); // pending node changes first, as a tick does
        if (c->n_rx != c->n) return fail(RM_ERR_STATE, "internal: the receiver table does not hold every node");
        rm_context::Hops &hp = c->hp;
        const size_t n = size_t(c->n);
        RM_TRY(grow(c, need(hp.words, 4), need(hp.off_list, n), need(hp.queue, n)));
        RM_HIP(hp.h.ensure());
        RM_HIP(hipMemsetAsync(hp.words.p, 0, 4 * sizeof(unsigned long long), c->stream));
        rm::HopDev h{};
        h.hop = out.hop;
        h.parent = out.parent;
        h.rssi = reinterpret_cast<uint64_t *>(out.rssi);
        h.children = out.children;
        h.queue = hp.queue.p;
        h.tail = reinterpret_cast<uint32_t *>(hp.words.p + 2);
        h.prep = hp.words.p;
        h.off_list = hp.off_list.p;
        h.min_rssi = min_rssi;
        const bool scan = nb_needs_scan(c);
        const rm::NodesDev nd = nodes_dev(c);
        const rm::ModelDev m = model_dev(c);
        CallProbe probe(c); // (rm_profile_kernels names the path that ran)
        // the tail after the launches enqueued so far
        auto tail = [&](int &count) -> int {
            RM_TRY(hp.h.read(c->stream, h.tail, sizeof(uint32_t)));
            count = int(std::min<uint32_t>(hp.h.low(), uint32_t(c->n)));
            return RM_OK;
        };
        // both directions walk as a receiver somewhere: HEARD_BY in the expansion (the frontier node receives), HEARS in the
        // parent pass -- k_nb_prep's words and list, once per query
        RM_HIP(rm::launch_nb_prep(c->stream, nd, hp.words.p, hp.off_list.p));
        RM_HIP(rm::launch_hop_seed(c->stream, nd, h, roots, n_roots));
        int lo = 0, hi = 0;
        RM_TRY(tail(hi));
        t.roots = hi;
        for (int level = 0; hi > lo; ++level) { // an empty frontier ends the query
            t.max_hop = level;
            RM_HIP(rm::launch_hop_expand(c->stream, nd, m, h, direction, scan, lo, hi, level));
            lo = hi;
            RM_TRY(tail(hi));
        }
        t.reached = hi;
        if ((out.parent || out.rssi || out.children) && t.reached > t.roots) {
            RM_HIP(rm::launch_hop_parent(c->stream, nd, m, h, direction, scan, t.roots, t.reached));
            RM_HIP(hipStreamSynchronize(c->stream));
        }
    }
    if (totals) *totals = t;
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_hops_query_device(rm_context *c, int32_t direction, double min_rssi_dbm, const int32_t *dev_roots, int32_t n_roots, const rm_hops_out *dev_out,
                         rm_hops_totals *totals)
{
    RM_TRY(hops_check(c, direction, min_rssi_dbm, dev_roots, n_roots, dev_out));
    RM_HIP(hipSetDevice(c->device));
    return hops_run(c, direction, min_rssi_dbm, dev_roots, n_roots, *dev_out, totals);
}

int rm_hops_query(rm_context *c, int32_t direction, double min_rssi_dbm, const int32_t *roots, int32_t n_roots, const rm_hops_out *out,
                  rm_hops_totals *totals)
{
    RM_TRY(hops_check(c, direction, min_rssi_dbm, roots, n_roots, out));
    RM_TRY(roots_in_table(roots, n_roots, c->n));
    if (c->n < 1) {
        if (totals) *totals = rm_hops_totals{0, -1, 0, 0};
        return RM_OK;
    }
    RM_HIP(hipSetDevice(c->device));
    // the call's device block lives for this call only: rssi, hop, parent, children, roots
    const size_t n = size_t(c->n);
    CallBlock b(c);
    const size_t o_rssi = b.reserve(n * 8), o_hop = b.reserve(n * 4), o_par = b.reserve(n * 4), o_chl = b.reserve(n * 4),
                 o_roots = b.reserve(size_t(std::max(n_roots, 1)) * 4);
    RM_TRY(b.alloc());
    const rm_hops_out dv{b.at<int32_t>(o_hop), b.at<int32_t>(o_par, out->parent), b.at<double>(o_rssi, out->rssi), b.at<int32_t>(o_chl, out->children)};
    int32_t *d_roots = b.at<int32_t>(o_roots);
    b.in(d_roots, roots, size_t(n_roots) * 4);
    const int rc = b.ok() ? hops_run(c, direction, min_rssi_dbm, d_roots, n_roots, dv, totals) : RM_OK;
    if (rc == RM_OK) {
        b.out(out->hop, dv.hop, n * 4);
        b.out(out->parent, dv.parent, n * 4);
        b.out(out->rssi, dv.rssi, n * 8);
        b.out(out->children, dv.children, n * 4);
    }
    return b.finish(rc, "rm_hops_query");
}

int rm_hops_next_device(rm_context *c, const int32_t *dev_parent, const int32_t *dev_src, int32_t n, int32_t *dev_want)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (n < 0 || (n > 0 && (!dev_parent || !dev_src || !dev_want))) return fail(RM_ERR_INVALID, "bad arguments");
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(rm::launch_hop_next(c->stream, dev_parent, c->n, dev_src, n, dev_want));
    return RM_OK;
}

int rm_hops_from_links(int32_t n_nodes, int32_t n_links, const int32_t *node, const int32_t *far, const double *rssi, double min_rssi_dbm,
                       const int32_t *roots, int32_t n_roots, const rm_hops_out *out, rm_hops_totals *totals)
{
    if (!out || !out->hop) return fail(RM_ERR_INVALID, "out or out->hop is NULL");
    if (n_nodes < 0 || n_links < 0 || n_roots < 0) return fail(RM_ERR_INVALID, "negative count");
    if (n_links > 0 && (!node || !far || !rssi)) return fail(RM_ERR_INVALID, "node, far or rssi is NULL");
    RM_TRY(roots_check(roots, n_roots));
    if (min_rssi_dbm != min_rssi_dbm) return fail(RM_ERR_INVALID, "min_rssi_dbm is NaN");
    for (int32_t i = 0; i < n_links; ++i)
        if (node[i] < 0 || node[i] >= n_nodes || far[i] < 0 || far[i] >= n_nodes) return fail(RM_ERR_INVALID, "link index out of range");
    RM_TRY(roots_in_table(roots, n_roots, n_nodes));
    const double nan = quiet_nan();
    for (int32_t j = 0; j < n_nodes; ++j) {
        out->hop[j] = -1;
        if (out->parent) out->parent[j] = -1;
        if (out->rssi) out->rssi[j] = nan;
        if (out->children) out->children[j] = 0;
    }
    // the links by their far end: a frontier node finds the nodes it may be the parent of
    auto is_link = [&](size_t i) { return node[i] != far[i] && rssi[i] >= min_rssi_dbm; }; // (a NaN rssi compares false)
    const ByFar g = by_far(size_t(n_nodes), size_t(n_links), is_link, [&](size_t i) { return far[i]; });
    rm_hops_totals t{0, -1, 0, 0};
    std::vector<int32_t> frontier, next;
    for (int32_t k = 0; k < n_roots; ++k)
        if (out->hop[roots[k]] == -1) {
            out->hop[roots[k]] = 0;
            frontier.push_back(roots[k]);
        }
    t.roots = int32_t(frontier.size());
    for (int32_t level = 0; !frontier.empty(); ++level) {
        t.max_hop = level;
        t.reached += int32_t(frontier.size());
        next.clear();
        for (const int32_t p : frontier)
            for (size_t k = g.first[size_t(p)]; k < g.first[size_t(p) + 1]; ++k) {
                const int32_t j = node[g.entry[k]];
                if (out->hop[j] == -1) {
                    out->hop[j] = level + 1;
                    next.push_back(j);
                }
            }
        frontier.swap(next);
    }
    if (out->parent || out->rssi || out->children) {
        // the best candidate one level closer, by the rule's order: rssi descending, then the smaller node index
        const std::vector<int32_t> best = best_by_rssi(n_nodes, n_links, node, far, rssi, [&](int32_t i) {
            return is_link(size_t(i)) && out->hop[node[i]] >= 1 && out->hop[far[i]] == out->hop[node[i]] - 1;
        });
        for (int32_t j = 0; j < n_nodes; ++j) {
            const int32_t b = best[size_t(j)];
            if (b < 0) continue;
            if (out->parent) out->parent[j] = far[b];
            if (out->rssi) out->rssi[j] = rssi[b];
            if (out->children) ++out->children[far[b]];
        }
    }
    if (totals) *totals = t;
    return RM_OK;
}

} // extern "C"
