// rm_stats.hip -- per-node traffic counters: a pass over the FINISHED result
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The pass reads what every result reader reads -- a slot's compact packet-major arrays with their final verdicts (after the
// draws, the SINR stages and the frame error model's pass) and the records of the tick's new frames -- and adds to one table of
// eight 64-bit counters per node.  It writes nothing else.  All sums are integers, so the table does not depend on the order of
// the additions, on how ticks were grouped into launches, or on packet numbers.
//
// Receiver side: one lane per heard link, up to three atomics into the receiver's record (receivers of a frame are distinct, so
// these spread over the table).  Transmitter side: the links are packet-major, so the links of a frame sit in consecutive lanes --
// run_prefix (rm_device.hpp) finds each run of one packet inside the wave, and the run's leading lane adds the run's length and
// its delivered count ONCE: a frame with 40 links issues one pair of atomics per wave it touches, not 80 to one address.
#include "rm_device.hpp"

namespace rm {

// Workgroups per slot, as the frame error model's pass: 16 384 lanes per stride over the slot's links (not tuned).
constexpr int kStatsBlocks = 64;

RM_D void stats_add(uint64_t *p, uint64_t v) { (void)atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v)); }

RM_D void stats_body(const StatsDev &sd, const TickDev &t)
{
    // an empty tick has no result and changes nothing
    if (!t.out_count || !t.out_verdict || !t.out_pkt || !t.out_dst || !t.tx) return;
    const int n_new = t.n_active - t.first_new;
    if (n_new <= 0) return;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    // a slot that overflowed its capacity or was dropped counts nothing (the frame error model's conditions)
    if (t.out_count[1] != 0u || (t.stage_count && t.stage_count[1] != 0u)) {
        if (first) stats_add(&sd.totals->ticks_skipped, 1u);
        return;
    }
    if (first) stats_add(&sd.totals->ticks_counted, 1u);
    const rm_tx_record *recs = t.tx + t.first_new;
    const int lane = int(threadIdx.x & 63u);
    const uint32_t stride = gridDim.x * blockDim.x; // (a multiple of 64, as every lane's first index is its wave's base + lane)
    const uint32_t n = min(t.out_count[0], t.out_count[2]);
    const uint32_t n_up = (n + 63u) & ~63u; // whole waves: every lane of a wave that has a link takes part in the ballots and shuffles
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        int key = -1; // lanes past the end, and links whose frame does not count: no run, no predicate
        int32_t src = -1;
        bool counts = false, delivered = false;
        if (i < n) {
            const int q = t.out_pkt[i];
            if (q >= 0 && q < n_new) {
                const rm_tx_record *rec = recs + q;
                src = rec->src;
                const uint64_t air = uint64_t(rec->air_us);
                const int32_t dst = t.out_dst[i];
                delivered = t.out_verdict[i] == uint8_t(RM_DELIVERED);
                if (dst >= 0 && dst < sd.n_nodes) { // (records and results may come from the caller: never outside the table)
                    rm_node_stats *r = sd.table + dst;
                    stats_add(&r->rx_heard, 1u);
                    stats_add(&r->rx_air_us, air);
                    if (delivered) stats_add(&r->rx_delivered, 1u);
                }
                counts = src >= 0 && src < sd.n_nodes;
                if (counts) key = q;
            }
        }
        const RunInfo heard = run_prefix(key, counts, lane);
        const RunInfo deliv = run_prefix(key, counts && delivered, lane);
        if (counts && lane == heard.start) { // (every lane of a run has the run's packet, so its source: the leader counts with all of them)
            rm_node_stats *r = sd.table + src;
            stats_add(&r->tx_links_heard, heard.total);
            if (deliv.total) stats_add(&r->tx_links_delivered, deliv.total);
        }
    }
    // the tick's new frames: padding, deferred candidates of the gates and CSMA slots not made have src -1
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < uint32_t(n_new); q += stride) {
        const int32_t src = recs[q].src;
        if (src < 0 || src >= sd.n_nodes) continue;
        rm_node_stats *r = sd.table + src;
        stats_add(&r->tx_frames, 1u);
        stats_add(&r->tx_air_us, uint64_t(recs[q].air_us));
        if (t.pkt_interference && t.pkt_interference[q]) stats_add(&r->tx_failed, 1u);
    }
}

__global__ void __launch_bounds__(256) k_stats(const StatsDev sd, const TickDev t) { stats_body(sd, t); }
__global__ void __launch_bounds__(256) k_stats_batch(const StatsDev sd, const TickDev *__restrict__ ticks) { stats_body(sd, ticks[blockIdx.y]); }

hipError_t launch_stats(hipStream_t s, const StatsDev &sd, const TickDev &t)
{
    RM_KLAUNCH(k_stats, dim3(kStatsBlocks), dim3(256), 0, s, sd, t);
    return hipGetLastError();
}

hipError_t launch_stats_batch(hipStream_t s, const StatsDev &sd, int n, const TickDev *dev_ticks)
{
    if (n < 1 || n > kMaxBatch) return hipErrorInvalidValue;
    RM_KLAUNCH(k_stats_batch, dim3(kStatsBlocks, n), dim3(256), 0, s, sd, dev_ticks);
    return hipGetLastError();
}

} // namespace rm
