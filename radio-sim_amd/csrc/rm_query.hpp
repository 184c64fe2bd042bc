// rm_query.hpp -- what the queries' translation units share (rm_api_neighbors.cpp, rm_api_hops.cpp, rm_api_routes.cpp,
// rm_api_etx.cpp): the device block a host form stages its call through, the refusals of a root
// list, the choice of the whole-table scan, the growth of a query's scratch, and, in plain C++ that touches no device, the graph
// passes of the pure forms.  Header-only: each of those files also compiles alone beside a stand-alone test program.
// (PinnedWords, the pinned block the queries read a few device words through, is in rm_host.hpp: the context holds three by value.)
#pragma once

#include "rm_host.hpp"

#include <functional>
#include <limits>
#include <queue>
#include <utility>

namespace rmh {

// ---- the device-backed forms

// The device block of one host-form call: the inputs and outputs as padded segments of ONE allocation that lives for the call.
//   reserve every segment -> alloc -> in(...) -> the launches, if ok() -> out(...) -> return finish(rc, "rm_xxx_query")
// finish waits for the stream whatever happened before -- a copy or a kernel may still use the block -- and only then frees it.
struct CallBlock {
    rm_context *c;
    char *d = nullptr;
    size_t bytes = 0;
    hipError_t e = hipSuccess; // the first copy that failed
    explicit CallBlock(rm_context *ctx) : c(ctx) {}
    // room for `b` bytes: the segment's offset
    size_t reserve(size_t b)
    {
        const size_t o = bytes;
        bytes += pad64(b);
        return o;
    }
    int alloc()
    {
        RM_HIP(hipMalloc(reinterpret_cast<void **>(&d), bytes));
        return RM_OK;
    }
    // the segment at `off` -- for an optional array: nullptr if the caller left `asked` out
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(d + off); }
    template <typename T> T *at(size_t off, const void *asked) const { return asked ? at<T>(off) : nullptr; }
    bool ok() const { return e == hipSuccess; }
    // host -> device and device -> host on the context's stream; a null pointer on either side is an array that is not there
    void in(void *dev, const void *host, size_t b)
    {
        if (ok() && dev && host && b) e = hipMemcpyAsync(dev, host, b, hipMemcpyHostToDevice, c->stream);
    }
    void out(void *host, const void *dev, size_t b)
    {
        if (ok() && dev && host && b) e = hipMemcpyAsync(host, dev, b, hipMemcpyDeviceToHost, c->stream);
    }
    // rc, or the HIP failure where everything else went well
    int finish(int rc, const char *who)
    {
        const hipError_t es = hipStreamSynchronize(c->stream); // (also on the way out of a failure: the block is freed below)
        if (e == hipSuccess) e = es;
        if (rc == RM_OK && e != hipSuccess) rc = fail(RM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
        (void)hipFree(d);
        d = nullptr;
        return rc;
    }
};

// what every form refuses of a root list
inline int roots_check(const int32_t *roots, int32_t n_roots)
{
    if (n_roots < 0) return fail(RM_ERR_INVALID, "negative root count");
    if (n_roots > 0 && !roots) return fail(RM_ERR_INVALID, "roots is NULL");
    return RM_OK;
}
// ... and of a list in host memory
inline int roots_in_table(const int32_t *roots, int32_t n_roots, int32_t n_nodes)
{
    for (int32_t k = 0; k < n_roots; ++k)
        if (roots[k] < 0 || roots[k] >= n_nodes) return fail(RM_ERR_INVALID, "root index out of range");
    return RM_OK;
}

// The walk over a node's potential links (rm_nbwalk.hpp) evaluates every pair of the table -- SCAN -- where the boxes bound
// nothing: on a table that is not sorted, in an fp32 frame beyond the plan's slack (LaunchCfg::f64_filter) and for a medium without
// a finite cut-off.  The neighbour, hop and route queries all choose it here.
inline bool nb_needs_scan(const rm_context *c) { return !c->rx_sorted || c->f32_slack > 0.05 || !(c->params.ld_exponent > 0.0); }

// A query's scratch: need(buffer, elements)..., and if any buffer is short the stream is synchronised once -- an earlier query
// may still read the old blocks -- and all are grown.
template <typename T> struct Need {
    DevBuf<T> &buf;
    size_t n;
};
template <typename T> Need<T> need(DevBuf<T> &buf, size_t n) { return Need<T>{buf, n}; }
template <typename... T> int grow(rm_context *c, Need<T>... needs)
{
    if (!((needs.buf.n < needs.n) || ...)) return RM_OK;
    RM_HIP(hipStreamSynchronize(c->stream));
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? needs.buf.ensure(needs.n) : e), ...);
    if (e != hipSuccess) return fail(RM_ERR_HIP, std::string("a query's scratch: ") + hipGetErrorString(e));
    return RM_OK;
}

// ---- the pure forms: plain C++, no device

// the NaN every form writes where there is no rssi
inline double quiet_nan()
{
    const uint64_t bits = 0x7FF8000000000000ull;
    double v;
    std::memcpy(&v, &bits, sizeof(v));
    return v;
}

// The entries of a list or table that count, by their far end (a counting sort): node p finds the entries it may be the parent's
// end of in entry[first[p] .. first[p + 1]), in the list's order.
struct ByFar {
    std::vector<size_t> first, entry;
};
template <typename Counts, typename Far> ByFar by_far(size_t n_nodes, size_t n_entries, Counts &&counts, Far &&far)
{
    ByFar g;
    g.first.assign(n_nodes + 1, 0);
    for (size_t i = 0; i < n_entries; ++i)
        if (counts(i)) ++g.first[size_t(far(i)) + 1];
    for (size_t p = 0; p < n_nodes; ++p) g.first[p + 1] += g.first[p];
    g.entry.assign(g.first[n_nodes], 0);
    std::vector<size_t> at(g.first.begin(), g.first.end() - 1);
    for (size_t i = 0; i < n_entries; ++i)
        if (counts(i)) g.entry[at[size_t(far(i))]++] = i;
    return g;
}

// Dijkstra from all roots at once over the entries of `g`: entry i leads from its far end to node near(i) at cost link_cost(i) > 0.
// Writes cost[0 .. n_nodes): UINT64_MAX where no root is reached.  Roots (inside the table) may repeat.
struct LeastCosts {
    int32_t roots = 0, reached = 0;
    uint64_t max_cost = 0;
};
template <typename Near, typename LinkCost>
LeastCosts least_costs(int32_t n_nodes, const ByFar &g, const int32_t *roots, int32_t n_roots, Near &&near, LinkCost &&link_cost, uint64_t *cost)
{
    const uint64_t unreached = std::numeric_limits<uint64_t>::max();
    LeastCosts t;
    for (int32_t j = 0; j < n_nodes; ++j) cost[j] = unreached;
    typedef std::pair<uint64_t, int32_t> Entry;
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    for (int32_t k = 0; k < n_roots; ++k)
        if (cost[roots[k]] == unreached) {
            cost[roots[k]] = 0;
            heap.push(Entry(0, roots[k]));
            ++t.roots;
        }
    while (!heap.empty()) {
        const Entry top = heap.top();
        heap.pop();
        const size_t p = size_t(top.second);
        if (top.first != cost[p]) continue; // (an entry from before the node's cost fell)
        ++t.reached;
        t.max_cost = std::max(t.max_cost, top.first);
        for (size_t k = g.first[p]; k < g.first[p + 1]; ++k) {
            const size_t i = g.entry[k];
            const int32_t j = near(i);
            const uint64_t nc = top.first + link_cost(i);
            if (nc < cost[j]) {
                cost[j] = nc;
                heap.push(Entry(nc, j));
            }
        }
    }
    return t;
}

// best[j]: among the links i of the list with node[i] == j for which candidate(i) holds, the first in the rule's order -- rssi
// descending, then the smaller far index --, -1 where there is none
template <typename Candidate>
std::vector<int32_t> best_by_rssi(int32_t n_nodes, int32_t n_links, const int32_t *node, const int32_t *far, const double *rssi, Candidate &&candidate)
{
    std::vector<int32_t> best(size_t(n_nodes), -1);
    for (int32_t i = 0; i < n_links; ++i) {
        if (!candidate(i)) continue;
        int32_t &b = best[size_t(node[i])];
        if (b < 0 || rssi[i] > rssi[b] || (rssi[i] == rssi[b] && far[i] < far[b])) b = i;
    }
    return best;
}

} // namespace rmh
