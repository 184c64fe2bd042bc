// rm_api_etx.cpp -- C ABI: the measured-route query, least path cost (ETX in units of 1/128) and parent toward a set of roots over
// the measured links of a watch table (the kernels are rm_etx.hip), and the pure host forms
// rm_etx_link_cost, rm_etx_combine and rm_etx_from_tables.
//
// The query READS a watch table -- the context's own (E14) or the caller's -- and writes the caller's outputs and scratch of its
// own (rm_context::Etx).  The node table, the model and the medium play no part.
#include "rm_query.hpp"
#include "rm_math.hpp"

using namespace rmh;

namespace rmh {

void etx_release(rm_context *c)
{
    c->etx.lc.release();
    c->etx.stamp.release();
    c->etx.words.release();
    c->etx.h.release();
}

static int etx_params_check(const rm_etx_params *p)
{
    if (!p) return fail(RM_ERR_INVALID, "params is NULL");
    if (p->mode != RM_ETX_INBOUND && p->mode != RM_ETX_BOTH) return fail(RM_ERR_INVALID, "mode is RM_ETX_INBOUND or RM_ETX_BOTH");
    if (p->reserved != 0 || p->reserved2 != 0) return fail(RM_ERR_INVALID, "reserved is not 0");
    if (p->min_heard > (1u << 31)) return fail(RM_ERR_INVALID, "min_heard is above 2^31");
    if (p->max_link_cost < 128u || p->max_link_cost > 65535u) return fail(RM_ERR_INVALID, "max_link_cost is outside 128 .. 65535");
    if (p->hysteresis > 65535u) return fail(RM_ERR_INVALID, "hysteresis is above 65535");
    return RM_OK;
}

// explicit tables: the struct's own rules (aligned: what the kernels' row loads need of device pointers)
static int etx_tables_check(const rm_etx_tables *t, bool aligned)
{
    if (t->K != 1 && t->K != 2 && t->K != 4 && t->K != 8) return fail(RM_ERR_INVALID, "K is 1, 2, 4 or 8");
    if (t->reserved != 0) return fail(RM_ERR_INVALID, "tables: reserved is not 0");
    if (!t->peer || !t->stats) return fail(RM_ERR_INVALID, "tables: peer or stats is NULL");
    if (aligned && (reinterpret_cast<uintptr_t>(t->peer) % (4u * unsigned(t->K)) != 0 || reinterpret_cast<uintptr_t>(t->stats) % 8u != 0))
        return fail(RM_ERR_INVALID, "tables: peer is not aligned to 4 K bytes or stats not to 8");
    return RM_OK;
}

// what both device forms refuse, before anything is launched
static int etx_check(rm_context *c, const rm_etx_params *p, const rm_etx_tables *t, bool aligned, const int32_t *roots, int32_t n_roots,
                     const rm_etx_out *out)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (!out || !out->cost) return fail(RM_ERR_INVALID, "out or out->cost is NULL");
    RM_TRY(etx_params_check(p));
    if (t) RM_TRY(etx_tables_check(t, aligned));
    RM_TRY(roots_check(roots, n_roots));
    if (c->in_tick) return fail(RM_ERR_STATE, "rm_etx_query between rm_tick_begin and rm_tick_flush");
    RM_TRY(graphs_refuse(c, "the measured-route query is not part of them"));
    if (!t) {
        if (!linkstats_on(c)) return fail(RM_ERR_STATE, "tables is NULL and the watched-link statistics are off");
        if (part_count(c) != c->n || part_spatial(c))
            return fail(RM_ERR_STATE, "tables is NULL on a context with a receiver partition: its watched-link statistics count nothing");
        if (c->lk.n != c->n) return fail(RM_ERR_STATE, "internal: the watch table does not hold every node");
    }
    return RM_OK;
}

// the whole query on the context's stream; t (or the context's tables), roots, cur and the arrays of `out` are device memory.
// Returns with the stream idle.
static int etx_run(rm_context *c, const rm_etx_params &p, const rm_etx_tables *t, const int32_t *roots, int32_t n_roots, const int32_t *cur,
                   const rm_etx_out &out, rm_etx_totals *totals)
{
    rm_etx_totals tt{0, 0, 0, 0, 0, 0, 0};
    if (c->n > 0) {
        rm_context::Etx &x = c->etx;
        rm::EtxDev e{};
        if (t) {
            e.peer = t->peer;
            e.stats = t->stats;
            e.K = t->K;
        } else {
            const rm::LinkStatsDev ld = linkstats_dev(c);
            e.peer = ld.peer;
            e.stats = ld.table;
            e.K = ld.K;
        }
        const size_t n = size_t(c->n), nk = n * size_t(e.K);
        RM_TRY(grow(c, need(x.lc, nk), need(x.stamp, n), need(x.words, size_t(rm::kEtxWords))));
        RM_HIP(x.h.ensure());
        RM_HIP(hipMemsetAsync(x.words.p, 0, size_t(rm::kEtxWords) * sizeof(unsigned long long), c->stream));
        e.lc = x.lc.p;
        e.stamp = x.stamp.p;
        e.cost = reinterpret_cast<unsigned long long *>(out.cost);
        e.parent = out.parent;
        e.slot = out.slot;
        e.link_cost = out.link_cost;
        e.children = out.children;
        e.cur = cur;
        e.words = x.words.p;
        e.n = c->n;
        e.mode = p.mode;
        e.min_heard = p.min_heard;
        e.max_link_cost = p.max_link_cost;
        e.hysteresis = p.hysteresis;
        CallProbe probe(c); // (rm_profile_kernels names what ran)
        RM_HIP(rm::launch_etx_cost(c->stream, e));
        RM_HIP(rm::launch_etx_seed(c->stream, e, roots, n_roots));
        x.last_rounds = 0;
        x.last_examined = 0;
        // a round that lowered nobody ends the query: the costs are a fixed point.  One launch, one 8-byte copy, one wait per round
        for (int round = 1; n_roots > 0; ++round) {
            RM_HIP(rm::launch_etx_relax(c->stream, e, round));
            RM_TRY(x.h.read(c->stream, e.words + (round & 1), sizeof(unsigned long long)));
            ++x.last_rounds;
            x.last_examined += uint64_t(x.h.p[0] >> 32);
            if (x.h.low() == 0u) break;
        }
        if (out.parent || out.slot || out.link_cost || out.children || cur) {
            if (out.children) RM_HIP(hipMemsetAsync(out.children, 0, n * sizeof(int32_t), c->stream));
            RM_HIP(rm::launch_etx_parent(c->stream, e));
        }
        RM_HIP(rm::launch_etx_totals(c->stream, e));
        RM_TRY(x.h.read(c->stream, e.words + 2, 6 * sizeof(unsigned long long)));
        const unsigned long long top = (unsigned long long)c->n, *w = x.h.p;
        tt.reached = int32_t(std::min(w[0], top));
        tt.max_cost = w[1];
        tt.roots = int32_t(std::min(w[2], top));
        tt.kept = int32_t(std::min(w[3], top));
        tt.switched = int32_t(std::min(w[4], top));
        tt.lost = int32_t(std::min(w[5], top));
    }
    if (totals) *totals = tt;
    return RM_OK;
}

// c(j, k) of every entry of a host table, 0 where the link does not count: k_etx_cost's text
static void etx_host_costs(int32_t n_nodes, const rm_etx_tables &t, const rm_etx_params &p, std::vector<uint32_t> &lc)
{
    const int K = t.K;
    auto inbound = [&](size_t at, uint32_t &c) { return rm::etx_entry_cost(p.min_heard, p.max_link_cost, t.stats[at].heard, t.stats[at].delivered, c); };
    lc.assign(size_t(n_nodes) * size_t(K), 0u);
    for (int32_t j = 0; j < n_nodes; ++j)
        for (int k = 0; k < K; ++k) {
            const size_t i = size_t(j) * size_t(K) + size_t(k);
            const int32_t q = t.peer[i];
            uint32_t c = 0u;
            if (q < 0 || q >= n_nodes || q == j || !inbound(i, c)) continue;
            if (p.mode == RM_ETX_BOTH) {
                int kr = -1;
                for (int s = K - 1; s >= 0; --s)
                    if (t.peer[size_t(q) * size_t(K) + size_t(s)] == j) kr = s;
                uint32_t cr = 0u;
                if (kr < 0 || !inbound(size_t(q) * size_t(K) + size_t(kr), cr)) continue;
                const uint64_t both = rm::etx_combine(c, cr);
                if (both > uint64_t(p.max_link_cost)) continue;
                c = uint32_t(both);
            }
            lc[i] = c;
        }
}

} // namespace rmh

extern "C" {

void rm_etx_defaults(rm_etx_params *p)
{
    if (!p) return;
    *p = rm_etx_params{RM_ETX_INBOUND, 0, 4u, 2048u, 192u, 0u};
}

int rm_etx_validate(const rm_etx_params *params) { return etx_params_check(params); }

int rm_etx_query_device(rm_context *c, const rm_etx_params *params, const rm_etx_tables *tables, const int32_t *dev_roots, int32_t n_roots,
                        const int32_t *dev_cur, const rm_etx_out *dev_out, rm_etx_totals *totals)
{
    RM_TRY(etx_check(c, params, tables, true, dev_roots, n_roots, dev_out));
    RM_HIP(hipSetDevice(c->device));
    return etx_run(c, *params, tables, dev_roots, n_roots, dev_cur, *dev_out, totals);
}

int rm_etx_query(rm_context *c, const rm_etx_params *params, const rm_etx_tables *tables, const int32_t *roots, int32_t n_roots, const int32_t *cur,
                 const rm_etx_out *out, rm_etx_totals *totals)
{
    RM_TRY(etx_check(c, params, tables, false, roots, n_roots, out));
    RM_TRY(roots_in_table(roots, n_roots, c->n));
    if (c->n < 1) {
        if (totals) *totals = rm_etx_totals{0, 0, 0, 0, 0, 0, 0};
        return RM_OK;
    }
    RM_HIP(hipSetDevice(c->device));
    // the call's device block lives for this call only: cost, parent, slot, link_cost, children, cur, roots, and the caller's tables
    const size_t n = size_t(c->n), nk = tables ? n * size_t(tables->K) : 0;
    CallBlock b(c);
    const size_t o_cost = b.reserve(n * 8), o_par = b.reserve(n * 4), o_slot = b.reserve(n * 4), o_lc = b.reserve(n * 4), o_chl = b.reserve(n * 4),
                 o_cur = b.reserve(n * 4), o_roots = b.reserve(size_t(std::max(n_roots, 1)) * 4), o_peer = b.reserve(nk * 4),
                 o_stats = b.reserve(nk * sizeof(rm_link_stats));
    RM_TRY(b.alloc());
    const rm_etx_out dv{b.at<uint64_t>(o_cost), b.at<int32_t>(o_par, out->parent), b.at<int32_t>(o_slot, out->slot),
                        b.at<uint32_t>(o_lc, out->link_cost), b.at<int32_t>(o_chl, out->children)};
    int32_t *d_cur = b.at<int32_t>(o_cur, cur), *d_roots = b.at<int32_t>(o_roots);
    rm_etx_tables dt{};
    if (tables) {
        dt = rm_etx_tables{b.at<int32_t>(o_peer), b.at<rm_link_stats>(o_stats), tables->K, 0};
        b.in(b.at<int32_t>(o_peer), tables->peer, nk * 4);
        b.in(b.at<rm_link_stats>(o_stats), tables->stats, nk * sizeof(rm_link_stats));
    }
    b.in(d_roots, roots, size_t(n_roots) * 4);
    b.in(d_cur, cur, n * 4);
    const int rc = b.ok() ? etx_run(c, *params, tables ? &dt : nullptr, d_roots, n_roots, d_cur, dv, totals) : RM_OK;
    if (rc == RM_OK) {
        b.out(out->cost, dv.cost, n * 8);
        b.out(out->parent, dv.parent, n * 4);
        b.out(out->slot, dv.slot, n * 4);
        b.out(out->link_cost, dv.link_cost, n * 4);
        b.out(out->children, dv.children, n * 4);
    }
    return b.finish(rc, "rm_etx_query");
}

int rm_etx_last_work(rm_context *c, int32_t *rounds, uint64_t *examined)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (rounds) *rounds = c->etx.last_rounds;
    if (examined) *examined = c->etx.last_examined;
    return RM_OK;
}

int rm_etx_link_cost(const rm_etx_params *params, uint64_t heard, uint64_t delivered, uint32_t *cost)
{
    if (etx_params_check(params) != RM_OK) return 0;
    uint32_t c = 0;
    if (!rm::etx_entry_cost(params->min_heard, params->max_link_cost, heard, delivered, c)) return 0;
    if (cost) *cost = c;
    return 1;
}

uint64_t rm_etx_combine(uint32_t c_in, uint32_t c_rev) { return rm::etx_combine(c_in, c_rev); }

int rm_etx_from_tables(int32_t n_nodes, const rm_etx_tables *tables, const rm_etx_params *params, const int32_t *roots, int32_t n_roots,
                       const int32_t *cur, const rm_etx_out *out, rm_etx_totals *totals)
{
    if (!out || !out->cost) return fail(RM_ERR_INVALID, "out or out->cost is NULL");
    RM_TRY(etx_params_check(params));
    if (!tables) return fail(RM_ERR_INVALID, "tables is NULL");
    RM_TRY(etx_tables_check(tables, false));
    if (n_nodes < 0 || n_roots < 0) return fail(RM_ERR_INVALID, "negative count");
    RM_TRY(roots_check(roots, n_roots));
    RM_TRY(roots_in_table(roots, n_roots, n_nodes));
    const uint64_t unreached = std::numeric_limits<uint64_t>::max();
    const int K = tables->K;
    std::vector<uint32_t> lc;
    etx_host_costs(n_nodes, *tables, *params, lc);
    // the counting entries by their far end -- a settled node finds the nodes it may be the parent of -- and Dijkstra over them
    const ByFar g = by_far(size_t(n_nodes), lc.size(), [&](size_t i) { return lc[i] != 0u; }, [&](size_t i) { return tables->peer[i]; });
    const LeastCosts found =
        least_costs(n_nodes, g, roots, n_roots, [&](size_t i) { return int32_t(i / size_t(K)); }, [&](size_t i) { return lc[i]; }, out->cost);
    rm_etx_totals t{found.reached, found.roots, 0, 0, 0, 0, found.max_cost};
    // the parents (k_etx_parent's text); cur[j] is read before parent[j] is written: the two may be one array
    if (out->children)
        for (int32_t j = 0; j < n_nodes; ++j) out->children[j] = 0;
    for (int32_t j = 0; j < n_nodes; ++j) {
        const uint64_t cj = out->cost[j];
        const int32_t q = cur ? cur[j] : -1;
        const bool valid = q >= 0 && q < n_nodes;
        int32_t par = -1;
        int sl = -1;
        uint32_t best = 0u;
        if (cj != 0 && cj != unreached) {
            const size_t row = size_t(j) * size_t(K);
            if (valid) {
                uint32_t bc = 0u;
                int bk = -1;
                for (int k = 0; k < K; ++k)
                    if (lc[row + size_t(k)] && tables->peer[row + size_t(k)] == q && (bk < 0 || lc[row + size_t(k)] < bc)) {
                        bc = lc[row + size_t(k)];
                        bk = k;
                    }
                if (bk >= 0 && out->cost[q] < cj && out->cost[q] + bc <= cj + params->hysteresis) {
                    par = q;
                    sl = bk;
                    best = bc;
                }
            }
            if (par < 0)
                for (int k = 0; k < K; ++k) {
                    const uint32_t c = lc[row + size_t(k)];
                    if (!c) continue;
                    const int32_t p = tables->peer[row + size_t(k)];
                    if (out->cost[p] != unreached && out->cost[p] + c == cj && (sl < 0 || rm::etx_precedes(c, p, k, best, par, sl))) {
                        par = p;
                        sl = k;
                        best = c;
                    }
                }
        }
        if (out->parent) out->parent[j] = par;
        if (out->slot) out->slot[j] = sl;
        if (out->link_cost) out->link_cost[j] = best;
        if (out->children && par >= 0) ++out->children[par];
        t.kept += par >= 0 && valid && par == q;
        t.switched += par >= 0 && valid && par != q;
        t.lost += cj == unreached && valid;
    }
    if (totals) *totals = t;
    return RM_OK;
}

} // extern "C"
