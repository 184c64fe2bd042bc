// rm_api_etx.cpp -- C ABI: the measured-route query, least path cost (ETX in units of 1/128) and parent toward a set of roots over
// the measured links of a watch table (the kernels are rm_etx.hip), and the pure host forms
// rm_etx_link_cost, rm_etx_combine and rm_etx_from_tables.
//
// The query READS a watch table -- the context's own (E14) or the caller's -- and writes the caller's outputs and scratch of its
// own (rm_context::Etx).  The node table, the model and the medium play no part.
#include "rm_host.hpp"
#include "rm_math.hpp"

#include <limits>
#include <queue>

using namespace rmh;

namespace rmh {

void etx_release(rm_context *c)
{
    c->etx.lc.release();
    c->etx.stamp.release();
    c->etx.words.release();
    if (c->etx.h_words) (void)hipHostFree(c->etx.h_words);
    c->etx.h_words = nullptr;
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
    if (n_roots < 0) return fail(RM_ERR_INVALID, "negative root count");
    if (n_roots > 0 && !roots) return fail(RM_ERR_INVALID, "roots is NULL");
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
        if (x.lc.n < nk || x.stamp.n < n || x.words.n < size_t(rm::kEtxWords) || !x.h_words) {
            RM_HIP(hipStreamSynchronize(c->stream)); // (an earlier query may still read the old blocks)
            RM_HIP(x.lc.ensure(nk));
            RM_HIP(x.stamp.ensure(n));
            RM_HIP(x.words.ensure(size_t(rm::kEtxWords)));
            if (!x.h_words) RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&x.h_words), 64, hipHostMallocMapped));
        }
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
            RM_HIP(hipMemcpyAsync(x.h_words, e.words + (round & 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            RM_HIP(hipStreamSynchronize(c->stream));
            ++x.last_rounds;
            x.last_examined += uint64_t(x.h_words[0] >> 32);
            if (uint32_t(x.h_words[0]) == 0u) break;
        }
        if (out.parent || out.slot || out.link_cost || out.children || cur) {
            if (out.children) RM_HIP(hipMemsetAsync(out.children, 0, n * sizeof(int32_t), c->stream));
            RM_HIP(rm::launch_etx_parent(c->stream, e));
        }
        RM_HIP(rm::launch_etx_totals(c->stream, e));
        RM_HIP(hipMemcpyAsync(x.h_words, e.words + 2, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        RM_HIP(hipStreamSynchronize(c->stream));
        const unsigned long long top = (unsigned long long)c->n;
        tt.reached = int32_t(std::min(x.h_words[0], top));
        tt.max_cost = x.h_words[1];
        tt.roots = int32_t(std::min(x.h_words[2], top));
        tt.kept = int32_t(std::min(x.h_words[3], top));
        tt.switched = int32_t(std::min(x.h_words[4], top));
        tt.lost = int32_t(std::min(x.h_words[5], top));
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
    for (int32_t k = 0; k < n_roots; ++k)
        if (roots[k] < 0 || roots[k] >= c->n) return fail(RM_ERR_INVALID, "root index out of range");
    if (c->n < 1) {
        if (totals) *totals = rm_etx_totals{0, 0, 0, 0, 0, 0, 0};
        return RM_OK;
    }
    RM_HIP(hipSetDevice(c->device));
    // the call's device block lives for this call only: cost, parent, slot, link_cost, children, cur, roots, and the caller's tables
    const size_t n = size_t(c->n), nk = tables ? n * size_t(tables->K) : 0;
    const size_t o_par = pad64(n * 8), o_slot = o_par + pad64(n * 4), o_lc = o_slot + pad64(n * 4), o_chl = o_lc + pad64(n * 4),
                 o_cur = o_chl + pad64(n * 4), o_roots = o_cur + pad64(n * 4), o_peer = o_roots + pad64(size_t(std::max(n_roots, 1)) * 4),
                 o_stats = o_peer + pad64(nk * 4), total = o_stats + pad64(nk * sizeof(rm_link_stats));
    char *d = nullptr;
    RM_HIP(hipMalloc(reinterpret_cast<void **>(&d), total));
    rm_etx_out dv{};
    dv.cost = reinterpret_cast<uint64_t *>(d);
    dv.parent = out->parent ? reinterpret_cast<int32_t *>(d + o_par) : nullptr;
    dv.slot = out->slot ? reinterpret_cast<int32_t *>(d + o_slot) : nullptr;
    dv.link_cost = out->link_cost ? reinterpret_cast<uint32_t *>(d + o_lc) : nullptr;
    dv.children = out->children ? reinterpret_cast<int32_t *>(d + o_chl) : nullptr;
    int32_t *d_cur = cur ? reinterpret_cast<int32_t *>(d + o_cur) : nullptr;
    int32_t *d_roots = reinterpret_cast<int32_t *>(d + o_roots);
    rm_etx_tables dt{};
    if (tables) dt = rm_etx_tables{reinterpret_cast<const int32_t *>(d + o_peer), reinterpret_cast<const rm_link_stats *>(d + o_stats), tables->K, 0};
    int rc = RM_OK;
    hipError_t e = hipSuccess;
    if (n_roots > 0) e = hipMemcpyAsync(d_roots, roots, size_t(n_roots) * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && cur) e = hipMemcpyAsync(d_cur, cur, n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && tables) e = hipMemcpyAsync(d + o_peer, tables->peer, nk * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && tables) e = hipMemcpyAsync(d + o_stats, tables->stats, nk * sizeof(rm_link_stats), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) rc = etx_run(c, *params, tables ? &dt : nullptr, d_roots, n_roots, d_cur, dv, totals);
    if (rc == RM_OK && e == hipSuccess) {
        e = hipMemcpyAsync(out->cost, dv.cost, n * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.parent) e = hipMemcpyAsync(out->parent, dv.parent, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.slot) e = hipMemcpyAsync(out->slot, dv.slot, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.link_cost) e = hipMemcpyAsync(out->link_cost, dv.link_cost, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && dv.children) e = hipMemcpyAsync(out->children, dv.children, n * 4, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream); // (also on the way out of a failure: the block is freed below)
    if (e == hipSuccess) e = es;
    if (rc == RM_OK && e != hipSuccess) rc = fail(RM_ERR_HIP, std::string("rm_etx_query: ") + hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
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
    if (n_roots > 0 && !roots) return fail(RM_ERR_INVALID, "roots is NULL");
    for (int32_t k = 0; k < n_roots; ++k)
        if (roots[k] < 0 || roots[k] >= n_nodes) return fail(RM_ERR_INVALID, "root index out of range");
    const uint64_t unreached = std::numeric_limits<uint64_t>::max();
    const int K = tables->K;
    std::vector<uint32_t> lc;
    etx_host_costs(n_nodes, *tables, *params, lc);
    // the counting entries by their far end (a counting sort): a settled node finds the nodes it may be the parent of
    std::vector<size_t> first(size_t(n_nodes) + 1, 0), by_far(lc.size(), 0);
    for (size_t i = 0; i < lc.size(); ++i)
        if (lc[i]) ++first[size_t(tables->peer[i]) + 1];
    for (int32_t p = 0; p < n_nodes; ++p) first[size_t(p) + 1] += first[size_t(p)];
    {
        std::vector<size_t> at(first.begin(), first.end() - 1);
        for (size_t i = 0; i < lc.size(); ++i)
            if (lc[i]) by_far[at[size_t(tables->peer[i])]++] = i;
    }
    // Dijkstra from all roots at once
    rm_etx_totals t{0, 0, 0, 0, 0, 0, 0};
    for (int32_t j = 0; j < n_nodes; ++j) out->cost[j] = unreached;
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
        for (size_t k = first[size_t(p)]; k < first[size_t(p) + 1]; ++k) {
            const size_t i = by_far[k];
            const int32_t j = int32_t(i / size_t(K));
            const uint64_t nc = top.first + lc[i];
            if (nc < out->cost[j]) {
                out->cost[j] = nc;
                heap.push(Entry(nc, j));
            }
        }
    }
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
