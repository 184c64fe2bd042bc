// rm_linkstats.hip -- watched-link statistics: a pass over the FINISHED result
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// Every node has K slots of watched peers (K = 1, 2, 4 or 8; the caller sets them) and one rm_link_stats per slot.  The pass reads
// what the traffic counters' pass reads -- a slot's compact packet-major arrays with their final verdicts (after the draws, the SINR
// stages, the frame error model's and the listening schedules' passes) and the records of the tick's new frames -- and adds every
// heard link whose source is a watched peer of its receiver to that (receiver, slot) entry.  It writes nothing else.
//
// One lane per heard link: pkt, then the record's src and start_us (the lanes of a packet's run read one record), then dst and the
// receiver's peer row as one aligned load of 4 K bytes (K = 8: 32 bytes, which the hardware splits into two 16-byte loads) -- a
// plain load, so the rows stay in L2 -- compared against src in registers.  Only a lane that matches goes on to rssi, sinr and the
// verdict and issues atomics: 64-bit integer adds and 64-bit signed min / max.  No float atomics: the sums are integers (q8 fixed
// point), so the table does not depend on the order of the additions, on how ticks were grouped into launches, or on packet numbers.
//
// No wave-level pre-reduction: the links are packet-major and the receivers of a frame are distinct, so the matches of a packet's
// run land on different rows of the table; two additions to one entry come from different packets only (the traffic counters'
// transmitter side, where a whole run adds to one record, is the opposite case).
#include "rm_device.hpp"

namespace rm {

int64_t host_linkstats_q8(double x) { return linkstats_q8(x); }

// Workgroups per slot, as the traffic counters' pass: 16 384 lanes per stride over the slot's links (not tuned).
constexpr int kLinkStatsBlocks = 64;

template <int K> struct alignas(4 * K) PeerRow {
    int32_t v[K];
};

RM_D void ls_add(uint64_t *p, uint64_t v) { (void)atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v)); }
// (a signed sum through the unsigned add: two's complement, the same 64 bits)
RM_D void ls_add(int64_t *p, int64_t v) { (void)atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v)); }
RM_D void ls_min(int64_t *p, int64_t v) { (void)atomicMin(reinterpret_cast<long long *>(p), static_cast<long long>(v)); }
RM_D void ls_max(int64_t *p, int64_t v) { (void)atomicMax(reinterpret_cast<long long *>(p), static_cast<long long>(v)); }

template <int K> RM_D void linkstats_body(const LinkStatsDev &ld, const TickDev &t)
{
    // an empty tick has no result and changes nothing
    if (!t.out_count || !t.out_verdict || !t.out_pkt || !t.out_dst || !t.tx) return;
    const int n_new = t.n_active - t.first_new;
    if (n_new <= 0) return;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    // a slot that overflowed its capacity or was dropped counts nothing (the traffic counters' conditions)
    if (t.out_count[1] != 0u || (t.stage_count && t.stage_count[1] != 0u)) {
        if (first) ls_add(&ld.totals->ticks_skipped, 1u);
        return;
    }
    if (first) ls_add(&ld.totals->ticks_counted, 1u);
    const rm_tx_record *recs = t.tx + t.first_new;
    const uint32_t n = min(t.out_count[0], t.out_count[2]);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int q = t.out_pkt[i];
        if (q < 0 || q >= n_new) continue;
        const int32_t src = recs[q].src;
        if (src < 0 || src >= ld.n_nodes) continue; // (records and results may come from the caller: never outside the tables)
        const int32_t dst = t.out_dst[i];
        if (dst < 0 || dst >= ld.n_nodes) continue;
        const size_t row = size_t(dst) * size_t(K);
        const PeerRow<K> peers = *reinterpret_cast<const PeerRow<K> *>(ld.peer + row);
        int slot = -1;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (peers.v[k] == src) slot = k; // (the non-negative peers of a row are distinct: at most one matches)
        if (slot < 0) continue;
        rm_link_stats *e = ld.table + row + size_t(slot);
        const int64_t start = recs[q].start_us;
        ls_add(&e->heard, 1u);
        if (t.out_verdict[i] == uint8_t(RM_DELIVERED)) ls_add(&e->delivered, 1u);
        if (t.out_rssi) ls_add(&e->rssi_q8_sum, linkstats_q8(t.out_rssi[i]));
        if (t.out_sinr) ls_add(&e->sinr_q8_sum, linkstats_q8(t.out_sinr[i])); // (only the SINR medium has the column)
        ls_min(&e->first_start_us, start);
        ls_max(&e->last_start_us, start);
    }
}

RM_D void linkstats_any(const LinkStatsDev &ld, const TickDev &t)
{
    switch (ld.K) { // (uniform over the launch)
    case 1: linkstats_body<1>(ld, t); break;
    case 2: linkstats_body<2>(ld, t); break;
    case 4: linkstats_body<4>(ld, t); break;
    case 8: linkstats_body<8>(ld, t); break;
    default: break;
    }
}

__global__ void __launch_bounds__(256) k_linkstats(const LinkStatsDev ld, const TickDev t) { linkstats_any(ld, t); }
__global__ void __launch_bounds__(256) k_linkstats_batch(const LinkStatsDev ld, const TickDev *__restrict__ ticks) { linkstats_any(ld, ticks[blockIdx.y]); }

// word w of a cleared entry {0, 0, 0, 0, INT64_MAX, INT64_MIN}
RM_D int64_t cleared_word(uint32_t w) { return w < 4u ? int64_t(0) : (w == 4u ? INT64_MAX : INT64_MIN); }

// new tables, or rm_linkstats_reset (peers == nullptr): every entry cleared, one 64-bit word per lane; every peer slot empty
__global__ void __launch_bounds__(256) k_linkstats_clear(int32_t *__restrict__ peers, rm_link_stats *__restrict__ table, size_t n_entries)
{
    const size_t stride = size_t(gridDim.x) * blockDim.x;
    for (size_t e = size_t(blockIdx.x) * blockDim.x + threadIdx.x; e < n_entries * 6u; e += stride) {
        reinterpret_cast<int64_t *>(table)[e] = cleared_word(uint32_t(e % 6u));
        if (peers && e < n_entries) peers[e] = -1;
    }
}

// rm_linkstats_watch: the watch rule, one lane per (row, slot).  Row r is for node nodes[r] (nodes == nullptr: node r).  A slot whose
// peer stays keeps its entry; one whose peer changes is written and its entry cleared.  A node is listed at most once (the host
// has validated the list), so no two lanes touch one slot.
__global__ void __launch_bounds__(256) k_linkstats_scatter(int32_t *__restrict__ peer, rm_link_stats *__restrict__ table, int n_nodes, int K,
                                                           const int32_t *__restrict__ nodes, int n, const int32_t *__restrict__ new_peers)
{
    const size_t stride = size_t(gridDim.x) * blockDim.x;
    for (size_t e = size_t(blockIdx.x) * blockDim.x + threadIdx.x; e < size_t(n) * size_t(K); e += stride) {
        const size_t r = e / size_t(K);
        const int32_t node = nodes ? nodes[r] : int32_t(r);
        if (node < 0 || node >= n_nodes) continue;
        const size_t at = size_t(node) * size_t(K) + (e - r * size_t(K));
        const int32_t want = new_peers[e];
        if (peer[at] == want) continue;
        peer[at] = want;
        int64_t *w = reinterpret_cast<int64_t *>(table + at);
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) w[k] = cleared_word(k);
    }
}

static bool linkstats_k_ok(int K) { return K == 1 || K == 2 || K == 4 || K == 8; }

hipError_t launch_linkstats(hipStream_t s, const LinkStatsDev &ld, const TickDev &t)
{
    if (!linkstats_k_ok(ld.K)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_linkstats, dim3(kLinkStatsBlocks), dim3(256), 0, s, ld, t);
    return hipGetLastError();
}

hipError_t launch_linkstats_batch(hipStream_t s, const LinkStatsDev &ld, int n, const TickDev *dev_ticks)
{
    if (n < 1 || n > kMaxBatch || !linkstats_k_ok(ld.K)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_linkstats_batch, dim3(kLinkStatsBlocks, n), dim3(256), 0, s, ld, dev_ticks);
    return hipGetLastError();
}

hipError_t launch_linkstats_clear(hipStream_t s, int32_t *peers, rm_link_stats *table, size_t n_entries)
{
    if (n_entries < 1) return hipSuccess;
    const int blocks = int(std::max<size_t>(1, std::min<size_t>(1024, (n_entries * 6u + 255u) / 256u)));
    RM_KLAUNCH(k_linkstats_clear, dim3(blocks), dim3(256), 0, s, peers, table, n_entries);
    return hipGetLastError();
}

hipError_t launch_linkstats_scatter(hipStream_t s, int32_t *peer, rm_link_stats *table, int n_nodes, int K, const int32_t *nodes, int n,
                                    const int32_t *new_peers)
{
    if (n < 1) return hipSuccess;
    if (!linkstats_k_ok(K)) return hipErrorInvalidValue;
    const int blocks = int(std::max<size_t>(1, std::min<size_t>(1024, (size_t(n) * size_t(K) + 255u) / 256u)));
    RM_KLAUNCH(k_linkstats_scatter, dim3(blocks), dim3(256), 0, s, peer, table, n_nodes, K, nodes, n, new_peers);
    return hipGetLastError();
}

} // namespace rm
