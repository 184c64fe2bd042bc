// rm_api_routes.cpp -- C ABI: the route query, least path cost (ETX in units of 1/128) and best parent toward a set of roots over
// the potential-link graph (the kernels are rm_routes.hip), and the pure host forms
// rm_routes_link_cost and rm_routes_from_links.
//
// The query READS the node table and the model and writes the caller's outputs and scratch of its own (rm_context::Routes): what
// the hop query leaves alone it leaves alone, and the hop query's scratch as well.  The context's frame error model plays no part:
// kind, us_per_bit and air_us are the query's own parameters.
#include "rm_host.hpp"
#include "rm_math.hpp"

#include <limits>
#include <queue>

using namespace rmh;

namespace rmh {

void routes_release(rm_context *c)
{
    c->rt.words.release();
    c->rt.off_list.release();
    c->rt.stamp.release();
    c->rt.queue.release();
    if (c->rt.h_words) (void)hipHostFree(c->rt.h_words);
    c->rt.h_words = nullptr;
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
    if (n_roots < 0) return fail(RM_ERR_INVALID, "negative root count");
    if (n_roots > 0 && !roots) return fail(RM_ERR_INVALID, "roots is NULL");
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
        if (rt.words.n < kWords || rt.off_list.n < n || rt.stamp.n < n || rt.queue.n < 2 * n || !rt.h_words) {
            RM_HIP(hipStreamSynchronize(c->stream)); // (an earlier query may still read the old blocks)
            RM_HIP(rt.words.ensure(kWords));
            RM_HIP(rt.off_list.ensure(n));
            RM_HIP(rt.stamp.ensure(n));
            RM_HIP(rt.queue.ensure(2 * n));
            if (!rt.h_words) RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&rt.h_words), 64, hipHostMallocMapped));
        }
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
        // the whole-table scan exactly where the neighbour query takes it (rm_api_neighbors.cpp)
        const bool scan = !c->rx_sorted || c->f32_slack > 0.05 || !(c->params.ld_exponent > 0.0);
        const rm::NodesDev nd = nodes_dev(c);
        CallProbe probe(c); // (rm_profile_kernels names the path that ran)
        // a queue's tail after the launches enqueued so far: one copy into the pinned word, one wait
        auto tail = [&](int which, int &count) -> int {
            RM_HIP(hipMemcpyAsync(rt.h_words, r.tail + which, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            RM_HIP(hipStreamSynchronize(c->stream));
            count = int(std::min<uint32_t>(*reinterpret_cast<const uint32_t *>(rt.h_words), uint32_t(c->n)));
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
            RM_HIP(hipMemcpyAsync(rt.h_words, r.sums, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            RM_HIP(hipStreamSynchronize(c->stream));
            t.reached = int32_t(std::min<unsigned long long>(rt.h_words[0], (unsigned long long)c->n));
            t.max_cost = rt.h_words[1];
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
    for (int32_t k = 0; k < n_roots; ++k)
        if (roots[k] < 0 || roots[k] >= c->n) return fail(RM_ERR_INVALID, "root index out of range");
    if (c->n < 1) {
        if (totals) *totals = rm_routes_totals{0, 0, 0};
        return RM_OK;
    }
    RM_HIP(hipSetDevice(c->device));
    // the call's device block lives for this call only: cost, rssi, parent, link_cost, children, roots
    const size_t n = size_t(c->n);
    const size_t o_rssi = pad64(n * 8), o_par = o_rssi + pad64(n * 8), o_lc = o_par + pad64(n * 4), o_chl = o_lc + pad64(n * 4),
                 o_roots = o_chl + pad64(n * 4);
    char *d = nullptr;
    RM_HIP(hipMalloc(reinterpret_cast<void **>(&d), o_roots + pad64(size_t(std::max(n_roots, 1)) * 4)));
    rm_routes_out dv{};
    dv.cost = reinterpret_cast<uint64_t *>(d);
    dv.rssi = out->rssi ? reinterpret_cast<double *>(d + o_rssi) : nullptr;
    dv.parent = out->parent ? reinterpret_cast<int32_t *>(d + o_par) : nullptr;
    dv.link_cost = out->link_cost ? reinterpret_cast<uint32_t *>(d + o_lc) : nullptr;
    dv.children = out->children ? reinterpret_cast<int32_t *>(d + o_chl) : nullptr;
    int32_t *d_roots = reinterpret_cast<int32_t *>(d + o_roots);
    int rc = RM_OK;
    hipError_t e = hipSuccess;
    if (n_roots > 0) e = hipMemcpyAsync(d_roots, roots, size_t(n_roots) * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) rc = routes_run(c, *params, d_roots, n_roots, dv, totals);
    if (rc == RM_OK && e == hipSuccess) {
        e = hipMemcpyAsync(out->cost, dv.cost, n * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.parent) e = hipMemcpyAsync(out->parent, dv.parent, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.rssi) e = hipMemcpyAsync(out->rssi, dv.rssi, n * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.link_cost) e = hipMemcpyAsync(out->link_cost, dv.link_cost, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.children) e = hipMemcpyAsync(out->children, dv.children, n * 4, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream); // (also on the way out of a failure: the block is freed below)
    if (e == hipSuccess) e = es;
    if (rc == RM_OK && e != hipSuccess) rc = fail(RM_ERR_HIP, std::string("rm_routes_query: ") + hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
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
    if (n_roots > 0 && !roots) return fail(RM_ERR_INVALID, "roots is NULL");
    for (int32_t i = 0; i < n_links; ++i)
        if (node[i] < 0 || node[i] >= n_nodes || far[i] < 0 || far[i] >= n_nodes) return fail(RM_ERR_INVALID, "link index out of range");
    for (int32_t k = 0; k < n_roots; ++k)
        if (roots[k] < 0 || roots[k] >= n_nodes) return fail(RM_ERR_INVALID, "root index out of range");
    const uint64_t unreached = std::numeric_limits<uint64_t>::max();
    uint64_t nan_bits = 0x7FF8000000000000ull;
    double nan;
    std::memcpy(&nan, &nan_bits, sizeof(nan));
    for (int32_t j = 0; j < n_nodes; ++j) {
        out->cost[j] = unreached;
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
    // the counting links by their far end (a counting sort): a settled node finds the nodes it may be the parent of
    std::vector<int32_t> first(size_t(n_nodes) + 1, 0);
    std::vector<int32_t> by_far(static_cast<size_t>(n_links), 0);
    for (int32_t i = 0; i < n_links; ++i)
        if (lc[size_t(i)]) ++first[size_t(far[i]) + 1];
    for (int32_t p = 0; p < n_nodes; ++p) first[size_t(p) + 1] += first[size_t(p)];
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for (int32_t i = 0; i < n_links; ++i)
            if (lc[size_t(i)]) by_far[size_t(at[size_t(far[i])]++)] = i;
    }
    // Dijkstra from all roots at once
    rm_routes_totals t{0, 0, 0};
    typedef std::pair<uint64_t, int32_t> Entry;
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    for (int32_t k = 0; k < n_roots; ++k)
        if (out->cost[roots[k]] == unreached) {
            out->cost[roots[k]] = 0;
            heap.push(Entry(0, roots[k]));
            ++t.roots;
        }
    while (!heap.empty()) {
        const Entry top = heap.top();
        heap.pop();
        const int32_t p = top.second;
        if (top.first != out->cost[p]) continue; // (an entry from before the node's cost fell)
        ++t.reached;
        t.max_cost = std::max(t.max_cost, top.first);
        for (int32_t k = first[size_t(p)]; k < first[size_t(p) + 1]; ++k) {
            const int32_t i = by_far[size_t(k)];
            const uint64_t nc = top.first + lc[size_t(i)];
            if (nc < out->cost[node[i]]) {
                out->cost[node[i]] = nc;
                heap.push(Entry(nc, node[i]));
            }
        }
    }
    if (out->parent || out->rssi || out->link_cost || out->children) {
        // the best candidate on a least-cost path, by the rule's order: rssi descending, then the smaller node index
        std::vector<int32_t> best(size_t(n_nodes), -1);
        for (int32_t i = 0; i < n_links; ++i) {
            if (!lc[size_t(i)]) continue;
            const int32_t j = node[i];
            if (out->cost[j] == 0 || out->cost[j] == unreached || out->cost[far[i]] == unreached) continue;
            if (out->cost[far[i]] + lc[size_t(i)] != out->cost[j]) continue;
            const int32_t b = best[size_t(j)];
            if (b < 0 || rssi[i] > rssi[b] || (rssi[i] == rssi[b] && far[i] < far[b])) best[size_t(j)] = i;
        }
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
