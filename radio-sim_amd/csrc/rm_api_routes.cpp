// rm_api_routes.cpp -- C ABI: the route query, least path cost (ETX in units of 1/128) and best parent toward a set of roots over
// the potential-link graph (the kernels are rm_routes.hip), and the pure host forms
// rm_routes_link_cost and rm_routes_from_links.
//
// The query READS the node table and the model and writes the caller's outputs and scratch of its own (rm_context::Routes): what
// the hop query leaves alone it leaves alone, and the hop query's scratch as well.  The context's frame error model plays no part:
// kind, us_per_bit and air_us are the query's own parameters.
#include "rm_query.hpp"
#include "rm_math.hpp"

using namespace rmh;

namespace rmh {

void routes_release(rm_context *c)
{
    c->rt.words.release();
    c->rt.off_list.release();
    c->rt.stamp.release();
    c->rt.queue.release();
    c->rt.h.release();
}

// the parameter rules of every form
static int routes_params_check(const rm_routes_params *p, bool with_direction)
{
    if (!p) return fail(RM_ERR_INVALID, "params is NULL");
    if (with_direction && p->direction != RM_NB_HEARD_BY && p->direction != RM_NB_HEARS)
        return fail(RM_ERR_INVALID, "direction is RM_NB_HEARD_BY or RM_NB_HEARS");
    if (p->kind != RM_EM_NONE && p->kind != RM_EM_OQPSK_250K) return fail(RM_ERR_INVALID, "unknown error model kind");
    if (p->reserved != 0) return fail(RM_ERR_INVALID, "reserved is not 0");
    if (!(p->us_per_bit > 0.0) || !(p->us_per_bit < std::numeric_limits<double>::infinity()))
        return fail(RM_ERR_INVALID, "us_per_bit is not finite and > 0");
    if (p->air_us < 0) return fail(RM_ERR_INVALID, "air_us is negative");
    if (p->min_rssi_dbm != p->min_rssi_dbm) return fail(RM_ERR_INVALID, "min_rssi_dbm is NaN");
    if (p->max_link_cost < 128u || p->max_link_cost > 65535u) return fail(RM_ERR_INVALID, "max_link_cost is outside 128 .. 65535");
    return RM_OK;
}

// 10 * det_log10(ld_noise_lin) with ld_noise_lin as rm_set_model derives it from the noise floor
static double routes_noise_db(double noise_dbm) { return 10.0 * rm::det_log10(rm::det_pow10(noise_dbm / 10.0)); }

// a link of this rssi counts (valid params)
static bool routes_cost(const rm_routes_params &p, double noise_db, double rssi, uint32_t &c)
{
    if (!(rssi >= p.min_rssi_dbm)) return false; // (a NaN rssi is no link)
    return rm::route_link_cost(p.kind, p.us_per_bit, p.air_us, noise_db, double(p.max_link_cost), rssi, c);
}

// what both device forms refuse, before anything is launched
static int routes_check(rm_context *c, const rm_routes_params *p, const int32_t *roots, int32_t n_roots, const rm_routes_out *out)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (!out || !out->cost) return fail(RM_ERR_INVALID, "out or out->cost is NULL");
    RM_TRY(routes_params_check(p, true));
    RM_TRY(roots_check(roots, n_roots));
    if (c->params.kind != RM_MODEL_LOGDIST)
        return fail(RM_ERR_STATE, "the route query walks links that have an rssi: only the log-distance medium computes one per link");
    if (c->in_tick) return fail(RM_ERR_STATE, "rm_routes_query between rm_tick_begin and rm_tick_flush");
    if (part_count(c) != c->n || part_spatial(c))
        return fail(RM_ERR_STATE, "the route query needs the whole receiver table: this context has a receiver partition");
    RM_TRY(graphs_refuse(c, "the route query is not part of them"));
    return RM_OK;
}

// the whole query on the context's stream; roots and the arrays of `out` are device memory.  Returns with the stream idle.
static int routes_run(rm_context *c, const rm_routes_params &p, const int32_t *roots, int32_t n_roots, const rm_routes_out &out,
                      rm_routes_totals *totals)
{
    rm_routes_totals t{0, 0, 0};
    if (c->n > 0) {
        RM_TRY(prepare_nodes(c)); // pending node changes first, as a tick does
        if (c->n_rx != c->n) return fail(RM_ERR_STATE, "internal: the receiver table does not hold every node");
        rm_context::Routes &rt = c->rt;
        const size_t n = size_t(c->n);
        constexpr size_t kWords = 5;
        RM_TRY(grow(c, need(rt.words, kWords), need(rt.off_list, n), need(rt.stamp, n), need(rt.queue, 2 * n)));
        RM_HIP(rt.h.ensure());
        RM_HIP(hipMemsetAsync(rt.words.p, 0, kWords * sizeof(unsigned long long), c->stream));
        const rm::ModelDev m = model_dev(c);
        rm::RouteDev r{};
        r.cost = reinterpret_cast<unsigned long long *>(out.cost);
        r.parent = out.parent;
        r.rssi = reinterpret_cast<uint64_t *>(out.rssi);
        r.link_cost = out.link_cost;
        r.children = out.children;
        r.stamp = rt.stamp.p;
        r.queue[0] = rt.queue.p;
        r.queue[1] = rt.queue.p + n;
        r.tail = reinterpret_cast<uint32_t *>(rt.words.p + 2);
        r.sums = rt.words.p + 3;
        r.prep = rt.words.p;
        r.off_list = rt.off_list.p;
        r.min_rssi = p.min_rssi_dbm;
        r.kind = p.kind;
        r.us_per_bit = p.us_per_bit;
        r.air_us = p.air_us;
        r.noise_db = 10.0 * rm::det_log10(m.ld_noise_lin);
        r.max_cost = double(p.max_link_cost);
        const bool scan = nb_needs_scan(c);
        const rm::NodesDev nd = nodes_dev(c);
        CallProbe probe(c); // (rm_profile_kernels names the path that ran)
        // a queue's tail after the launches enqueued so far
        auto tail = [&](int which, int &count) -> int {
            RM_TRY(rt.h.read(c->stream, r.tail + which, sizeof(uint32_t)));
            count = int(std::min<uint32_t>(rt.h.low(), uint32_t(c->n)));
            return RM_OK;
        };
        // both directions walk as a receiver somewhere: HEARD_BY in the relaxation (the frontier node receives), HEARS in the
        // parent pass -- k_nb_prep's words and list, once per query
        RM_HIP(rm::launch_nb_prep(c->stream, nd, rt.words.p, rt.off_list.p));
        RM_HIP(rm::launch_route_seed(c->stream, nd, r, roots, n_roots));
        int count = 0;
        RM_TRY(tail(0, count));
        t.roots = count;
        rt.last_rounds = 0;
        rt.last_entries = 0;
        for (int round = 0; count > 0; ++round) { // an empty frontier ends the query: the costs are a fixed point
            ++rt.last_rounds;
            rt.last_entries += uint64_t(count);
            RM_HIP(rm::launch_route_relax(c->stream, nd, m, r, p.direction, scan, count, round));
            RM_TRY(tail((round & 1) ^ 1, count));
        }
        if (t.roots > 0) {
            if (out.parent || out.rssi || out.link_cost || out.children) RM_HIP(rm::launch_route_parent(c->stream, nd, m, r, p.direction, scan));
            RM_HIP(rm::launch_route_totals(c->stream, r, c->n));
            RM_TRY(rt.h.read(c->stream, r.sums, 2 * sizeof(unsigned long long)));
            t.reached = int32_t(std::min<unsigned long long>(rt.h.p[0], (unsigned long long)c->n));
            t.max_cost = rt.h.p[1];
        }
    }
    if (totals) *totals = t;
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_routes_query_device(rm_context *c, const rm_routes_params *params, const int32_t *dev_roots, int32_t n_roots, const rm_routes_out *dev_out,
                           rm_routes_totals *totals)
{
    RM_TRY(routes_check(c, params, dev_roots, n_roots, dev_out));
    RM_HIP(hipSetDevice(c->device));
    return routes_run(c, *params, dev_roots, n_roots, *dev_out, totals);
}

int rm_routes_query(rm_context *c, const rm_routes_params *params, const int32_t *roots, int32_t n_roots, const rm_routes_out *out,
                    rm_routes_totals *totals)
{
    RM_TRY(routes_check(c, params, roots, n_roots, out));
    RM_TRY(roots_in_table(roots, n_roots, c->n));
    if (c->n < 1) {
        if (totals) *totals = rm_routes_totals{0, 0, 0};
        return RM_OK;
    }
    RM_HIP(hipSetDevice(c->device));
    // the call's device block lives for this call only: cost, rssi, parent, link_cost, children, roots
    const size_t n = size_t(c->n);
    CallBlock b(c);
    const size_t o_cost = b.reserve(n * 8), o_rssi = b.reserve(n * 8), o_par = b.reserve(n * 4), o_lc = b.reserve(n * 4), o_chl = b.reserve(n * 4),
                 o_roots = b.reserve(size_t(std::max(n_roots, 1)) * 4);
    RM_TRY(b.alloc());
    const rm_routes_out dv{b.at<uint64_t>(o_cost), b.at<int32_t>(o_par, out->parent), b.at<double>(o_rssi, out->rssi),
                           b.at<uint32_t>(o_lc, out->link_cost), b.at<int32_t>(o_chl, out->children)};
    int32_t *d_roots = b.at<int32_t>(o_roots);
    b.in(d_roots, roots, size_t(n_roots) * 4);
    const int rc = b.ok() ? routes_run(c, *params, d_roots, n_roots, dv, totals) : RM_OK;
    if (rc == RM_OK) {
        b.out(out->cost, dv.cost, n * 8);
        b.out(out->parent, dv.parent, n * 4);
        b.out(out->rssi, dv.rssi, n * 8);
        b.out(out->link_cost, dv.link_cost, n * 4);
        b.out(out->children, dv.children, n * 4);
    }
    return b.finish(rc, "rm_routes_query");
}

int rm_routes_last_work(rm_context *c, int32_t *rounds, uint64_t *entries)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (rounds) *rounds = c->rt.last_rounds;
    if (entries) *entries = c->rt.last_entries;
    return RM_OK;
}

int rm_routes_link_cost(const rm_routes_params *params, double noise_dbm, double rssi, uint32_t *cost)
{
    if (routes_params_check(params, false) != RM_OK) return 0;
    uint32_t c = 0;
    if (!routes_cost(*params, routes_noise_db(noise_dbm), rssi, c)) return 0;
    if (cost) *cost = c;
    return 1;
}

int rm_routes_from_links(int32_t n_nodes, int32_t n_links, const int32_t *node, const int32_t *far, const double *rssi, const rm_routes_params *params,
                         double noise_dbm, const int32_t *roots, int32_t n_roots, const rm_routes_out *out, rm_routes_totals *totals)
{
    if (!out || !out->cost) return fail(RM_ERR_INVALID, "out or out->cost is NULL");
    RM_TRY(routes_params_check(params, false));
    if (n_nodes < 0 || n_links < 0 || n_roots < 0) return fail(RM_ERR_INVALID, "negative count");
    if (n_links > 0 && (!node || !far || !rssi)) return fail(RM_ERR_INVALID, "node, far or rssi is NULL");
    RM_TRY(roots_check(roots, n_roots));
    for (int32_t i = 0; i < n_links; ++i)
        if (node[i] < 0 || node[i] >= n_nodes || far[i] < 0 || far[i] >= n_nodes) return fail(RM_ERR_INVALID, "link index out of range");
    RM_TRY(roots_in_table(roots, n_roots, n_nodes));
    const uint64_t unreached = std::numeric_limits<uint64_t>::max();
    const double nan = quiet_nan();
    for (int32_t j = 0; j < n_nodes; ++j) {
        if (out->parent) out->parent[j] = -1;
        if (out->rssi) out->rssi[j] = nan;
        if (out->link_cost) out->link_cost[j] = 0;
        if (out->children) out->children[j] = 0;
    }
    // every entry's cost, 0 where it is no counting link
    const double noise_db = routes_noise_db(noise_dbm);
    std::vector<uint32_t> lc(static_cast<size_t>(n_links), 0u);
    for (int32_t i = 0; i < n_links; ++i) {
        uint32_t c = 0;
        if (node[i] != far[i] && routes_cost(*params, noise_db, rssi[i], c)) lc[size_t(i)] = c;
    }
    // the counting links by their far end -- a settled node finds the nodes it may be the parent of -- and Dijkstra over them
    const ByFar g = by_far(size_t(n_nodes), lc.size(), [&](size_t i) { return lc[i] != 0u; }, [&](size_t i) { return far[i]; });
    const LeastCosts found = least_costs(n_nodes, g, roots, n_roots, [&](size_t i) { return node[i]; }, [&](size_t i) { return lc[i]; }, out->cost);
    const rm_routes_totals t{found.reached, found.roots, found.max_cost};
    if (out->parent || out->rssi || out->link_cost || out->children) {
        // the best candidate on a least-cost path, by the rule's order: rssi descending, then the smaller node index
        const std::vector<int32_t> best = best_by_rssi(n_nodes, n_links, node, far, rssi, [&](int32_t i) {
            const uint64_t cj = out->cost[node[i]], cf = out->cost[far[i]];
            return lc[size_t(i)] && cj != 0 && cj != unreached && cf != unreached && cf + lc[size_t(i)] == cj;
        });
        for (int32_t j = 0; j < n_nodes; ++j) {
            const int32_t b = best[size_t(j)];
            if (b < 0) continue;
            if (out->parent) out->parent[j] = far[b];
            if (out->rssi) out->rssi[j] = rssi[b];
            if (out->link_cost) out->link_cost[j] = lc[size_t(b)];
            if (out->children) ++out->children[far[b]];
        }
    }
    if (totals) *totals = t;
    return RM_OK;
}

} // extern "C"
