// rm_routes.hip -- the route query: least path cost (ETX, in units of 1/128) and best parent toward a set of roots over the
// potential-link graph
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The hop query's structure (rm_hops.hip) with relaxation in place of claiming: a frontier of nodes whose cost fell, one launch per
// round, and one parent-selection pass behind the last round.  Both walk a node's pairs with nb_walk (rm_nbwalk.hpp), E16's walk;
// the seeding and the parent's choice are the hop query's too (nb_seed, NbBest), the queue append everybody's (wave_append).
// A node's cost only ever falls (a 64-bit atomicMin), and whoever lowers it queues it for the next round, at most once per round (a
// per-node round stamp): a queue never holds more than n_nodes entries.  Link costs are positive integers, so the rounds end, and
// the fixed point they end in does not depend on the order of the relaxations.
#include "rm_nbwalk.hpp"

namespace rm {

constexpr unsigned long long kRouteUnreached = ~0ull;

RM_D bool route_cost(const RouteDev &r, const double rssi, uint32_t &c)
{
    return route_link_cost(r.kind, r.us_per_bit, r.air_us, r.noise_db, r.max_cost, rssi, c);
}

// the outputs as "nothing reached": every later kernel only writes what a reached node gets
__global__ void __launch_bounds__(kBlock) k_route_init(const RouteDev r, const int n)
{
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    r.cost[i] = kRouteUnreached;
    r.stamp[i] = 0u;
    if (r.parent) r.parent[i] = -1;
    if (r.rssi) r.rssi[i] = kNbNoRssi;
    if (r.link_cost) r.link_cost[i] = 0u;
    if (r.children) r.children[i] = 0;
}

// the roots get cost 0 (nb_seed; the claim is an atomicCAS).  The claimed ones are frontier 0: queue[0][0 .. tail[0]).
__global__ void __launch_bounds__(kBlock) k_route_seed(const RouteDev r, const int n, const int32_t *__restrict__ roots, const int n_roots)
{
    nb_seed(roots, n_roots, n, &r.tail[0], r.queue[0], [&](const int node) { return atomicCAS(&r.cost[node], kRouteUnreached, 0ull) == kRouteUnreached; });
}

// One round: a wave per frontier node p = queue[round & 1][e] walks p's pairs in the REVERSE role, as k_hop_expand does -- DIR is
// the tree's direction, so the frontier node is the far end of the links it offers.  A lane whose pair is a counting link lowers the
// far end's cost to cost[p] + c; a lane that did lower it queues the far end for the next round unless somebody has already (the
// stamp).  cost[p] may fall while this wave runs, and it may be a stale, higher value from this CU's L1 if it fell earlier in this
// launch: whoever lowered p has queued p again, so the lower value is offered in the next round.  A far end that cost[p] + 128
// cannot lower is dropped before the pair's arithmetic (a stale high cost[far] costs the arithmetic and an atomicMin that lowers
// nothing).
template <int DIR, bool SCAN>
__global__ void __launch_bounds__(kBlock) k_route_relax(const NodesDev nd, const ModelDev m, const RouteDev r, const int count, const int round)
{
    const int lane = threadIdx.x & 63;
    const int in = round & 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) r.tail[in] = 0u; // (this round's count came as an argument; the next round appends here)
    const int e = int(blockIdx.x) * kNbWaves + wave_index();
    if (e >= count) return;
    const int p = uniform_i(r.queue[in][e]);
    if (uint32_t(p) >= uint32_t(nd.n)) return; // (cannot happen: the queues hold node indices)
    const unsigned long long cp = r.cost[p];
    if (cp == kRouteUnreached) return;         // (cannot happen: a queued node has a cost)
    const double cut = fmax(m.ld_sens, r.min_rssi);
    const uint32_t next = uint32_t(round) + 1u;
    int32_t *const out = r.queue[in ^ 1];
    uint32_t *const out_tail = r.tail + (in ^ 1);
    constexpr int WALK = DIR == RM_NB_HEARD_BY ? RM_NB_HEARS : RM_NB_HEARD_BY;
    nb_walk<WALK, SCAN>(
        nd, m, r.prep, r.off_list, p, cut, lane, [&](const int far) { return r.cost[far] > cp + 128ull; },
        [&](const bool link, const double rssi, const int far) {
            bool won = false;
            uint32_t c = 0u;
            if (link && route_cost(r, rssi, c)) {
                const unsigned long long nc = cp + c;
                if (atomicMin(&r.cost[far], nc) > nc) won = atomicMax(&r.stamp[far], next) < next;
            }
            wave_append(won, out_tail, out, far, uint32_t(nd.n), lane); // (one entry per node and round: always below n)
        });
}

// The parents: a wave per node j of the table; a reached node that is no root walks its pairs in the forward direction; the
// candidates are the counting links with cost[far] + c == cost[j].  Every lane keeps the best of its own pairs by the rule's order,
// the wave-wide best follows (NbBest, as in k_hop_parent), lane 0 writes.  The costs are final: the last round has ended.
template <int DIR, bool SCAN>
__global__ void __launch_bounds__(kBlock) k_route_parent(const NodesDev nd, const ModelDev m, const RouteDev r)
{
    const int lane = threadIdx.x & 63;
    const int j = int(blockIdx.x) * kNbWaves + wave_index();
    if (j >= nd.n) return;
    const unsigned long long cj = r.cost[j];
    if (cj == 0ull || cj == kRouteUnreached) return; // (wave-uniform: one address)
    const double cut = fmax(m.ld_sens, r.min_rssi);
    NbBest best; // (its word: the link's cost)
    nb_walk<DIR, SCAN>(
        nd, m, r.prep, r.off_list, j, cut, lane, [&](const int far) { return r.cost[far] <= cj - 128ull; },
        [&](const bool link, const double rssi, const int far) {
            uint32_t c = 0u;
            if (link && route_cost(r, rssi, c) && r.cost[far] + c == cj) best.offer(rssi, far, c);
        });
    best.wave<true>();
    if (lane == 0 && best.valid) {
        if (r.parent) r.parent[j] = best.node;
        if (r.rssi) r.rssi[j] = f2u(best.rssi);
        if (r.link_cost) r.link_cost[j] = best.word;
        if (r.children) atomicAdd(&r.children[best.node], 1);
    }
}

// reached and max_cost: a grid-stride pass over the final costs (wave_cost_totals), one pair of atomics per wave
__global__ void __launch_bounds__(kBlock) k_route_totals(const RouteDev r, const int n)
{
    const CostTotals t = wave_cost_totals(r.cost, n, kRouteUnreached);
    if ((threadIdx.x & 63) == 0 && t.reached) {
        atomicAdd(&r.sums[0], t.reached);
        atomicMax(&r.sums[1], t.max);
    }
}

hipError_t launch_route_seed(hipStream_t s, const NodesDev &nd, const RouteDev &r, const int32_t *roots, int n_roots)
{
    if (nd.n < 1) return hipSuccess;
    RM_KLAUNCH(k_route_init, dim3(cdiv(nd.n, kBlock)), dim3(kBlock), 0, s, r, nd.n);
    if (n_roots > 0) RM_KLAUNCH(k_route_seed, dim3(max(1, min(cdiv(n_roots, kBlock), 64))), dim3(kBlock), 0, s, r, nd.n, roots, n_roots);
    return hipGetLastError();
}

hipError_t launch_route_relax(hipStream_t s, const NodesDev &nd, const ModelDev &m, const RouteDev &r, int direction, bool scan, int count, int round)
{
    if (count < 1) return hipSuccess;
    const dim3 grid(cdiv(count, kNbWaves)), block(kBlock);
    RM_NB_BY_DIR_SCAN(k_route_relax, grid, block, nd, m, r, count, round);
    return hipGetLastError();
}

hipError_t launch_route_parent(hipStream_t s, const NodesDev &nd, const ModelDev &m, const RouteDev &r, int direction, bool scan)
{
    if (nd.n < 1) return hipSuccess;
    const dim3 grid(cdiv(nd.n, kNbWaves)), block(kBlock);
    RM_NB_BY_DIR_SCAN(k_route_parent, grid, block, nd, m, r);
    return hipGetLastError();
}

hipError_t launch_route_totals(hipStream_t s, const RouteDev &r, int n)
{
    if (n < 1) return hipSuccess;
    RM_KLAUNCH(k_route_totals, dim3(max(1, min(cdiv(n, kBlock), 256))), dim3(kBlock), 0, s, r, n);
    return hipGetLastError();
}

} // namespace rm
