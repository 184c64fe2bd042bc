// rm_etx.hip -- the measured-route query: least path cost (ETX, in units of 1/128) and parent toward a set of roots over a watch
// table's measured links
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The graph is the table: row j names j's candidate parents, and there is no reverse adjacency.  So the relaxation PULLS: one
// launch per round, a lane per node, and a node looks at its row only when one of its peers was lowered in the round before (a
// per-node round stamp).  Every node writes only its own words -- cost[j], stamp[j] -- so no atomic takes part in the costs, and
// correctness rests on launch boundaries alone: what a round reads of another node is what the rounds before it stored, or, if
// that node is being lowered in this very round, possibly the older, higher value.  A value read stale is merely too high, and
// its writer's new stamp makes every reader look again in the next round; link costs are positive integers, so the rounds end in
// the least fixed point whatever was read when (DESIGN.md 4.26 has the argument in full).
// The stats records (48 bytes, 16 of which matter) are read once, by k_etx_cost; the rounds and the parent pass read the 4-byte
// link costs it leaves.  All arithmetic is integer arithmetic.  No kernel here uses LDS or scratch memory.
#include "rm_device.hpp"

namespace rm {

constexpr unsigned long long kEtxUnreached = ~0ull;

// a node's row of peers or of link costs as one aligned load of 4 K bytes
template <int K> struct alignas(4 * K) EtxPeers {
    int32_t v[K];
};
template <int K> struct alignas(4 * K) EtxCosts {
    uint32_t v[K];
};

// INBOUND's rule for entry `at`
RM_D bool etx_inbound(const EtxDev &e, const size_t at, uint32_t &c)
{
    return etx_entry_cost(e.min_heard, e.max_link_cost, e.stats[at].heard, e.stats[at].delivered, c);
}

// c(j, k) of every entry, 0 where the link does not count: a lane per entry.  BOTH looks the reverse entry up here -- row p as
// one load, its lowest slot that holds j -- so that nothing behind this pass knows about modes.
template <int K> __global__ void __launch_bounds__(kBlock) k_etx_cost(const EtxDev e)
{
    const size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= size_t(e.n) * K) return;
    const int32_t j = int32_t(i / K);
    const int32_t p = e.peer[i];
    uint32_t c = 0u;
    bool counts = uint32_t(p) < uint32_t(e.n) && p != j && etx_inbound(e, i, c);
    if (counts && e.mode == RM_ETX_BOTH) {
        const EtxPeers<K> row = *reinterpret_cast<const EtxPeers<K> *>(e.peer + size_t(p) * K);
        int kr = -1;
#pragma unroll
        for (int s = K - 1; s >= 0; --s)
            if (row.v[s] == j) kr = s; // (descending: the lowest slot stays)
        uint32_t cr = 0u;
        counts = kr >= 0 && etx_inbound(e, size_t(p) * K + size_t(kr), cr);
        if (counts) {
            const uint64_t both = etx_combine(c, cr);
            counts = both <= uint64_t(e.max_link_cost);
            c = uint32_t(both);
        }
    }
    e.lc[i] = counts ? c : 0u;
}

__global__ void __launch_bounds__(kBlock) k_etx_init(const EtxDev e)
{
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= e.n) return;
    e.cost[i] = kEtxUnreached;
    e.stamp[i] = 0u;
}

// the roots: cost 0, stamp 1.  A root listed twice is written twice with the same words; an entry outside the table is skipped.
__global__ void __launch_bounds__(kBlock) k_etx_seed(const EtxDev e, const int32_t *__restrict__ roots, const int n_roots)
{
    for (int i = int(blockIdx.x * blockDim.x + threadIdx.x); i < n_roots; i += int(gridDim.x * blockDim.x)) {
        const int32_t node = roots[i];
        if (uint32_t(node) < uint32_t(e.n)) {
            e.cost[node] = 0ull;
            e.stamp[node] = 1u;
        }
    }
}

// One round.  lc[j][k] != 0 implies that peer[j][k] is a node index other than j (k_etx_cost, over the same table), so the
// reads of stamp and cost stay inside their arrays.  One atomicAdd per wave that examined a node, behind a ballot.
template <int K> __global__ void __launch_bounds__(kBlock) k_etx_relax(const EtxDev e, const uint32_t round)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) e.words[(round & 1u) ^ 1u] = 0ull; // (the next round's counter: nobody else touches it now)
    const int j = int(blockIdx.x * blockDim.x + threadIdx.x);
    bool look = false, lowered = false;
    if (j < e.n) {
        const unsigned long long cj = e.cost[j]; // (its own word: what the rounds before stored)
        if (cj != 0ull) {                        // (a root stays at 0)
            const EtxPeers<K> pr = *reinterpret_cast<const EtxPeers<K> *>(e.peer + size_t(j) * K);
            const EtxCosts<K> cr = *reinterpret_cast<const EtxCosts<K> *>(e.lc + size_t(j) * K);
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (cr.v[k] && e.stamp[pr.v[k]] == round) look = true;
            if (look) {
                unsigned long long best = kEtxUnreached;
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (cr.v[k]) {
                        const unsigned long long cp = e.cost[pr.v[k]];
                        if (cp != kEtxUnreached && cp + cr.v[k] < best) best = cp + cr.v[k];
                    }
                if (best < cj) {
                    e.cost[j] = best;
                    e.stamp[j] = round + 1u;
                    lowered = true;
                }
            }
        }
    }
    // (every wave gets here whole: no lane has returned)
    const uint64_t lm = ballot64(look), wm = ballot64(lowered);
    if (lm && (threadIdx.x & 63) == 0)
        (void)atomicAdd(&e.words[round & 1u], (static_cast<unsigned long long>(__popcll(lm)) << 32) | static_cast<unsigned long long>(__popcll(wm)));
}

// The parents, a lane per node, behind the last round (the costs are final).  cur[j] is read before parent[j] is written and no
// other node's entry of either is read: the two may be one buffer.  Roots and unreached nodes get -1, -1, 0.
template <int K> __global__ void __launch_bounds__(kBlock) k_etx_parent(const EtxDev e)
{
    const int j = int(blockIdx.x * blockDim.x + threadIdx.x);
    bool kept = false, switched = false, lost = false;
    if (j < e.n) {
        const unsigned long long cj = e.cost[j];
        const int32_t q = e.cur ? e.cur[j] : -1;
        const bool valid = uint32_t(q) < uint32_t(e.n);
        int32_t par = -1;
        int sl = -1;
        uint32_t lc = 0u;
        if (cj != 0ull && cj != kEtxUnreached) {
            const EtxPeers<K> pr = *reinterpret_cast<const EtxPeers<K> *>(e.peer + size_t(j) * K);
            const EtxCosts<K> cr = *reinterpret_cast<const EtxCosts<K> *>(e.lc + size_t(j) * K);
            if (valid) { // the keep rule: q's cheapest counting slot, the lower one of two equal ones
                uint32_t bc = 0u;
                int bk = -1;
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (cr.v[k] && pr.v[k] == q && (bk < 0 || cr.v[k] < bc)) {
                        bc = cr.v[k];
                        bk = k;
                    }
                if (bk >= 0) {
                    const unsigned long long cq = e.cost[q];
                    if (cq < cj && cq + bc <= cj + e.hysteresis) { // (an unreached q fails cq < cj)
                        par = q;
                        sl = bk;
                        lc = bc;
                    }
                }
            }
            if (par < 0) { // the best rule: the least (c, p, k) among the links on a least-cost path
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (cr.v[k]) {
                        const int32_t p = pr.v[k];
                        const unsigned long long cp = e.cost[p];
                        if (cp != kEtxUnreached && cp + cr.v[k] == cj && (sl < 0 || etx_precedes(cr.v[k], p, k, lc, par, sl))) {
                            par = p;
                            sl = k;
                            lc = cr.v[k];
                        }
                    }
            }
        }
        if (e.parent) e.parent[j] = par;
        if (e.slot) e.slot[j] = sl;
        if (e.link_cost) e.link_cost[j] = lc;
        if (e.children && par >= 0) (void)atomicAdd(&e.children[par], 1);
        kept = par >= 0 && valid && par == q;
        switched = par >= 0 && valid && par != q;
        lost = cj == kEtxUnreached && valid;
    }
    const uint64_t km = ballot64(kept), sm = ballot64(switched), om = ballot64(lost);
    if ((threadIdx.x & 63) == 0) {
        if (km) (void)atomicAdd(&e.words[5], static_cast<unsigned long long>(__popcll(km)));
        if (sm) (void)atomicAdd(&e.words[6], static_cast<unsigned long long>(__popcll(sm)));
        if (om) (void)atomicAdd(&e.words[7], static_cast<unsigned long long>(__popcll(om)));
    }
}

// reached, max_cost and roots: a grid-stride pass over the final costs (wave_cost_totals), one set of atomics per wave
__global__ void __launch_bounds__(kBlock) k_etx_totals(const EtxDev e)
{
    const CostTotals t = wave_cost_totals(e.cost, e.n, kEtxUnreached);
    if ((threadIdx.x & 63) == 0 && t.reached) {
        (void)atomicAdd(&e.words[2], t.reached);
        (void)atomicMax(&e.words[3], t.max);
        if (t.zeros) (void)atomicAdd(&e.words[4], t.zeros);
    }
}

// one launch of a kernel that is a template of K over `items` lanes
#define RM_ETX_BY_K(kern, items, ...)                                                                               \
    do {                                                                                                            \
        const dim3 grid_(static_cast<unsigned>(((items) + size_t(kBlock) - 1) / size_t(kBlock))), block_(kBlock);   \
        if (e.K == 1) RM_KLAUNCH(kern<1>, grid_, block_, 0, s, __VA_ARGS__);                                        \
        else if (e.K == 2) RM_KLAUNCH(kern<2>, grid_, block_, 0, s, __VA_ARGS__);                                   \
        else if (e.K == 4) RM_KLAUNCH(kern<4>, grid_, block_, 0, s, __VA_ARGS__);                                   \
        else if (e.K == 8) RM_KLAUNCH(kern<8>, grid_, block_, 0, s, __VA_ARGS__);                                   \
        else return hipErrorInvalidValue;                                                                           \
    } while (0)

hipError_t launch_etx_cost(hipStream_t s, const EtxDev &e)
{
    if (e.n < 1) return hipSuccess;
    RM_ETX_BY_K(k_etx_cost, size_t(e.n) * size_t(e.K), e);
    return hipGetLastError();
}

hipError_t launch_etx_seed(hipStream_t s, const EtxDev &e, const int32_t *roots, int n_roots)
{
    if (e.n < 1) return hipSuccess;
    RM_KLAUNCH(k_etx_init, dim3(cdiv(e.n, kBlock)), dim3(kBlock), 0, s, e);
    if (n_roots > 0) RM_KLAUNCH(k_etx_seed, dim3(max(1, min(cdiv(n_roots, kBlock), 64))), dim3(kBlock), 0, s, e, roots, n_roots);
    return hipGetLastError();
}

hipError_t launch_etx_relax(hipStream_t s, const EtxDev &e, int round)
{
    if (e.n < 1) return hipSuccess;
    RM_ETX_BY_K(k_etx_relax, size_t(e.n), e, uint32_t(round));
    return hipGetLastError();
}

hipError_t launch_etx_parent(hipStream_t s, const EtxDev &e)
{
    if (e.n < 1) return hipSuccess;
    RM_ETX_BY_K(k_etx_parent, size_t(e.n), e);
    return hipGetLastError();
}

hipError_t launch_etx_totals(hipStream_t s, const EtxDev &e)
{
    if (e.n < 1) return hipSuccess;
    RM_KLAUNCH(k_etx_totals, dim3(max(1, min(cdiv(e.n, kBlock), 256))), dim3(kBlock), 0, s, e);
    return hipGetLastError();
}

} // namespace rm
