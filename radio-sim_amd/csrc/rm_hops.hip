// rm_hops.hip -- the hop query: hop count and best parent toward a set of roots over the potential-link graph (DESIGN.md
// section 6, E17, and 4.22); the gather that turns the parents into the want list of the unicast outcome query
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// A level-synchronous frontier expansion, one launch per level, and one parent-selection pass behind the last level.  Both walk
// a node's pairs with nb_walk (rm_nbwalk.hpp), E16's walk.  The labelled nodes stand in ONE queue in the order they were claimed:
// level L's nodes are a contiguous range of it, which is that level's frontier and, for L >= 1, part of the parent pass's list.
// The order inside a level depends on the launch; no output does.
#include "rm_nbwalk.hpp"

namespace rm {

// the outputs as "nothing reached": every later kernel only writes what a labelled node gets
__global__ void __launch_bounds__(kBlock) k_hop_init(const HopDev h, const int n)
{
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    h.hop[i] = -1;
    if (h.parent) h.parent[i] = -1;
    if (h.rssi) h.rssi[i] = kNbNoRssi;
    if (h.children) h.children[i] = 0;
}

// the roots get hop 0 (nb_seed; the claim is an atomicCAS).  The claimed ones are frontier 0: queue[0 .. *tail), *tail zeroed in
// front of the launch.
__global__ void __launch_bounds__(kBlock) k_hop_seed(const HopDev h, const int n, const int32_t *__restrict__ roots, const int n_roots)
{
    nb_seed(roots, n_roots, n, h.tail, h.queue, [&](const int node) { return atomicCAS(&h.hop[node], -1, 0) == -1; });
}

// One level: a wave per frontier node p = queue[lo + e] (hop[p] == level) walks p's pairs in the REVERSE role -- DIR is the
// tree's direction, the link between a node and its parent seen from the node, so the frontier node is the far end.  HEARD_BY:
// the child transmits and p receives (E16's HEARS walk from p); HEARS: p transmits and the child receives (E16's HEARD_BY walk
// from p).  A lane whose pair is a link claims an unlabelled far end; the winners are appended to the queue behind *tail, one
// atomicAdd per wave.  Whoever claims a node gives it the same level.  A far end that is labelled already is dropped before the
// pair's arithmetic (a stale -1 from this CU's L1 costs the arithmetic and a compare-and-swap that fails, nothing else).
template <int DIR, bool SCAN>
__global__ void __launch_bounds__(kBlock) k_hop_expand(const NodesDev nd, const ModelDev m, const HopDev h, const int lo, const int hi, const int level)
{
    const int lane = threadIdx.x & 63;
    const int e = lo + int(blockIdx.x) * kNbWaves + wave_index();
    if (e >= hi) return;
    const int p = uniform_i(h.queue[e]);
    if (uint32_t(p) >= uint32_t(nd.n)) return; // (cannot happen: the queue holds claimed node indices)
    const double cut = fmax(m.ld_sens, h.min_rssi);
    constexpr int WALK = DIR == RM_NB_HEARD_BY ? RM_NB_HEARS : RM_NB_HEARD_BY;
    nb_walk<WALK, SCAN>(
        nd, m, h.prep, h.off_list, p, cut, lane, [&](const int far) { return h.hop[far] == -1; },
        [&](const bool link, const double, const int far) {
            const bool won = link && atomicCAS(&h.hop[far], -1, level + 1) == -1;
            wave_append(won, h.tail, h.queue, far, uint32_t(nd.n), lane); // (one entry per node: always below n)
        });
}

// The parents: a wave per reached non-root node j = queue[lo + e] walks j's pairs in the forward direction; the candidates are
// the links whose far end is one level closer.  Every lane keeps the best of its own pairs by the rule's order, the wave-wide
// best follows (NbBest), lane 0 writes.  The hops are complete: the last level's launch has ended.
template <int DIR, bool SCAN>
__global__ void __launch_bounds__(kBlock) k_hop_parent(const NodesDev nd, const ModelDev m, const HopDev h, const int lo, const int hi)
{
    const int lane = threadIdx.x & 63;
    const int e = lo + int(blockIdx.x) * kNbWaves + wave_index();
    if (e >= hi) return;
    const int j = uniform_i(h.queue[e]);
    if (uint32_t(j) >= uint32_t(nd.n)) return;
    const int up = uniform_i(h.hop[j]) - 1;
    const double cut = fmax(m.ld_sens, h.min_rssi);
    NbBest best;
    nb_walk<DIR, SCAN>(
        nd, m, h.prep, h.off_list, j, cut, lane, [&](const int far) { return h.hop[far] == up; },
        [&](const bool link, const double rssi, const int far) {
            if (link) best.offer(rssi, far, 0u);
        });
    best.wave<false>();
    if (lane == 0 && best.valid) {
        if (h.parent) h.parent[j] = best.node;
        if (h.rssi) h.rssi[j] = f2u(best.rssi);
        if (h.children) atomicAdd(&h.children[best.node], 1);
    }
}

// want[i] = parent[src[i]], -1 for a source outside the table (rm_hops_next_device)
__global__ void __launch_bounds__(kBlock) k_hop_next(const int32_t *__restrict__ parent, const int n_nodes, const int32_t *__restrict__ src, const int n,
                                                    int32_t *__restrict__ want)
{
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int s = src[i];
    want[i] = uint32_t(s) < uint32_t(n_nodes) ? parent[s] : -1;
}

hipError_t launch_hop_seed(hipStream_t s, const NodesDev &nd, const HopDev &h, const int32_t *roots, int n_roots)
{
    if (nd.n < 1) return hipSuccess;
    RM_KLAUNCH(k_hop_init, dim3(cdiv(nd.n, kBlock)), dim3(kBlock), 0, s, h, nd.n);
    if (n_roots > 0) RM_KLAUNCH(k_hop_seed, dim3(max(1, min(cdiv(n_roots, kBlock), 64))), dim3(kBlock), 0, s, h, nd.n, roots, n_roots);
    return hipGetLastError();
}

hipError_t launch_hop_expand(hipStream_t s, const NodesDev &nd, const ModelDev &m, const HopDev &h, int direction, bool scan, int lo, int hi, int level)
{
    if (hi <= lo) return hipSuccess;
    const dim3 grid(cdiv(hi - lo, kNbWaves)), block(kBlock);
    RM_NB_BY_DIR_SCAN(k_hop_expand, grid, block, nd, m, h, lo, hi, level);
    return hipGetLastError();
}

hipError_t launch_hop_parent(hipStream_t s, const NodesDev &nd, const ModelDev &m, const HopDev &h, int direction, bool scan, int lo, int hi)
{
    if (hi <= lo) return hipSuccess;
    const dim3 grid(cdiv(hi - lo, kNbWaves)), block(kBlock);
    RM_NB_BY_DIR_SCAN(k_hop_parent, grid, block, nd, m, h, lo, hi);
    return hipGetLastError();
}

hipError_t launch_hop_next(hipStream_t s, const int32_t *parent, int n_nodes, const int32_t *src, int n, int32_t *want)
{
    if (n < 1) return hipSuccess;
    RM_KLAUNCH(k_hop_next, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, parent, n_nodes, src, n, want);
    return hipGetLastError();
}

} // namespace rm
