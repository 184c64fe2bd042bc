// rm_nbtable.hip -- neighbour tables: discover, evict and expire watched peers on the device
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The tables are the watched-link statistics' (peer and rm_link_stats, [n_nodes][K]); the feature adds one 32-byte row of counters
// and one 64-bit word of scratch per node.  Nothing may depend on the order in which atomics land, so an update is cut into launches
// each of which READS only what the launch before it finished and what no lane of its own writes (the floods' discipline):
//   update   k_nbt_bid      a lane per link: the packet from pkt_offset, its source s, the receiver d and d's peer row as one aligned
//                           load of 4 K bytes; a lane whose link bids issues one 64-bit integer atomicMax over bid[d].  Reads the
//                           tables, writes the scratch
//            k_nbt_settle   a lane per node: 8 bytes of scratch; only a node with a bid reads its row's entries, chooses the slot
//                           (nbt_settle of rm_math.hpp, on the row as the bid pass saw it), writes peer[d][k] = s and the cleared
//                           entry, and puts a refused node's word back to rest
//            k_nbt_count    a lane per link again: the links from an admitted s to its d -- the word of d still names s -- are added
//                           to the fresh entry by the watched links' atomics (64-bit integer add, signed min / max)
//            k_nbt_rest     a lane per node: the scratch back to rest (the small launch over the nodes, not an epoch in the word: a
//                           key has 63 bits of (qc, s) and no room for one)
//   expire   k_nbt_expire   a lane per node walks its K slots; plain stores, the row is the lane's own
// Receivers of one frame are distinct, so the lanes of a packet's run hit different words and different entries.  The totals -- one
// address for everybody -- are added once per wave (relay_total).  No float atomics, no LDS beyond relay_total's shuffles, no
// scratch memory.
#include "rm_device.hpp"

namespace rm {

constexpr int kNbtThreads = kRelayThreads;
// Workgroups per pass over the slot's links, as the traffic counters', the watched links' and the floods' passes: 16 384 lanes per
// stride (not tuned)
constexpr int kNbtBlocks = 64;

template <int K> struct alignas(4 * K) NbtRow {
    int32_t v[K];
};

// the slot of row d that holds s, or -1: the row as one aligned load
template <int K> RM_D int nbt_find(const int32_t *peer, int d, int32_t s)
{
    const NbtRow<K> row = *reinterpret_cast<const NbtRow<K> *>(peer + size_t(d) * size_t(K));
    int slot = -1;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (row.v[k] == s) slot = k;
    return slot;
}
RM_D int nbt_find_any(const NbTableDev &f, int d, int32_t s)
{
    switch (f.K) { // (uniform over the launch)
    case 1: return nbt_find<1>(f.peer, d, s);
    case 2: return nbt_find<2>(f.peer, d, s);
    case 4: return nbt_find<4>(f.peer, d, s);
    default: return nbt_find<8>(f.peer, d, s);
    }
}

RM_D void nbt_add(uint64_t *p, uint64_t v) { (void)atomicAdd(reinterpret_cast<u64 *>(p), u64(v)); }
RM_D void nbt_add(int64_t *p, int64_t v) { (void)atomicAdd(reinterpret_cast<u64 *>(p), u64(v)); } // (two's complement: the same 64 bits)

__global__ void __launch_bounds__(kNbtThreads) k_nbt_init(const NbTableDev f)
{
    const int j = int(blockIdx.x) * kNbtThreads + int(threadIdx.x);
    if (j == 0) *f.totals = rm_nbtable_totals{};
    if (j >= f.n_nodes) return;
    f.node[j] = rm_nbtable_node{};
    f.bid[j] = 0ull;
}

__global__ void __launch_bounds__(kNbtThreads) k_nbt_bid(const NbTableDev f, const UcSlot s)
{
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (relay_slot_lost(s)) { // (uniform)
        if (first) atomicAdd(relay_w(&f.totals->skipped_slots), 1ull);
        return;
    }
    if (first) atomicAdd(relay_w(&f.totals->updates), 1ull);
    if (!s.rssi) return; // (no column: no link bids)
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t n = relay_links(s);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int32_t src = s.recs[relay_pkt(s, i)].src;
        const int32_t dst = s.dst[i];
        if (!relay_in(f, src) || !relay_in(f, dst) || src == dst) continue;
        if (nbt_find_any(f, dst, src) >= 0) continue;
        const double rssi = s.rssi[i];
        if (!nbt_bids(f.p, rssi, s.verdict[i] == uint8_t(RM_DELIVERED))) continue;
        atomicMax(relay_w(&f.bid[dst]), u64(nbt_key(rssi, src)));
    }
}

__global__ void __launch_bounds__(kNbtThreads) k_nbt_settle(const NbTableDev f, const int64_t time_us, const int32_t *__restrict__ pin)
{
    const int d = int(blockIdx.x) * kNbtThreads + int(threadIdx.x);
    u64 t_adm = 0, t_stale = 0, t_poor = 0, t_ref = 0;
    if (d < f.n_nodes) {
        const uint64_t key = f.bid[d];
        if (key != 0ull) {
            const size_t row = size_t(d) * size_t(f.K);
            int kind = 0;
            const int k = nbt_settle(f.p, f.n_nodes, f.K, d, f.peer + row, f.table + row, time_us, pin ? pin[d] : -1, kind);
            rm_nbtable_node &r = f.node[d];
            if (k < 0) {
                f.bid[d] = 0ull; // (the count pass sees no admission here)
                r.refused += 1u;
                t_ref = 1ull;
            } else {
                f.peer[row + size_t(k)] = nbt_key_src(key);
                nbt_clear(f.table[row + size_t(k)]);
                r.admitted += 1u;
                t_adm = 1ull;
                if (kind == 1) {
                    r.evicted_stale += 1u;
                    t_stale = 1ull;
                } else if (kind == 2) {
                    r.evicted_poor += 1u;
                    t_poor = 1ull;
                }
            }
        }
    }
    relay_total(&f.totals->admitted, t_adm);
    relay_total(&f.totals->evicted_stale, t_stale);
    relay_total(&f.totals->evicted_poor, t_poor);
    relay_total(&f.totals->refused, t_ref);
}

__global__ void __launch_bounds__(kNbtThreads) k_nbt_count(const NbTableDev f, const UcSlot s)
{
    if (relay_slot_lost(s)) return; // (uniform)
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t n = relay_links(s);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const rm_tx_record &rec = s.recs[relay_pkt(s, i)];
        const int32_t src = rec.src;
        const int32_t dst = s.dst[i];
        if (!relay_in(f, src) || !relay_in(f, dst)) continue;
        const uint64_t key = f.bid[dst];
        if (key == 0ull || nbt_key_src(key) != src) continue;
        const int k = nbt_find_any(f, dst, src);
        if (k < 0) continue; // (never: the settle launch wrote it)
        rm_link_stats *e = f.table + size_t(dst) * size_t(f.K) + size_t(k);
        const int64_t start = rec.start_us;
        nbt_add(&e->heard, 1u);
        if (s.verdict[i] == uint8_t(RM_DELIVERED)) nbt_add(&e->delivered, 1u);
        if (s.rssi) nbt_add(&e->rssi_q8_sum, linkstats_q8(s.rssi[i]));
        if (s.sinr) nbt_add(&e->sinr_q8_sum, linkstats_q8(s.sinr[i])); // (only the SINR medium has the column)
        (void)atomicMin(reinterpret_cast<long long *>(&e->first_start_us), (long long)start);
        (void)atomicMax(reinterpret_cast<long long *>(&e->last_start_us), (long long)start);
    }
}

__global__ void __launch_bounds__(kNbtThreads) k_nbt_rest(const NbTableDev f)
{
    const int d = int(blockIdx.x) * kNbtThreads + int(threadIdx.x);
    if (d < f.n_nodes && f.bid[d] != 0ull) f.bid[d] = 0ull;
}

__global__ void __launch_bounds__(kNbtThreads) k_nbt_expire(const NbTableDev f, const int64_t time_us, const int32_t *__restrict__ pin)
{
    const int d = int(blockIdx.x) * kNbtThreads + int(threadIdx.x);
    u64 t_exp = 0;
    if (d < f.n_nodes) {
        const size_t row = size_t(d) * size_t(f.K);
        const int32_t pn = pin ? pin[d] : -1;
        const bool pinned = relay_in(f, pn);
        for (int k = 0; k < f.K; ++k) {
            const int32_t peer = f.peer[row + size_t(k)];
            if (nbt_empty(f.n_nodes, d, peer) || (pinned && peer == pn)) continue;
            if (!nbt_stale(f.p.timeout_us, time_us, f.table[row + size_t(k)].last_start_us)) continue;
            f.peer[row + size_t(k)] = -1;
            nbt_clear(f.table[row + size_t(k)]);
            t_exp += 1ull;
        }
        if (t_exp) f.node[d].expired += uint32_t(t_exp);
    }
    relay_total(&f.totals->expired, t_exp);
}

// ---- launches

static bool nbt_dev_ok(const NbTableDev &f)
{
    return f.peer && f.table && f.node && f.totals && f.bid && f.n_nodes >= 1 && (f.K == 1 || f.K == 2 || f.K == 4 || f.K == 8);
}

hipError_t launch_nbtable_init(hipStream_t s, const NbTableDev &f)
{
    if (!f.node || !f.totals || !f.bid || f.n_nodes < 1) return hipErrorInvalidValue;
    RM_KLAUNCH(k_nbt_init, dim3(relay_blocks(f.n_nodes)), dim3(kNbtThreads), 0, s, f);
    return hipGetLastError();
}

hipError_t launch_nbtable_update(hipStream_t s, const NbTableDev &f, const UcSlot &slot, int64_t time_us, const int32_t *pin)
{
    if (!nbt_dev_ok(f) || time_us < 0) return hipErrorInvalidValue;
    RM_KLAUNCH(k_nbt_bid, dim3(kNbtBlocks), dim3(kNbtThreads), 0, s, f, slot);
    RM_KLAUNCH(k_nbt_settle, dim3(relay_blocks(f.n_nodes)), dim3(kNbtThreads), 0, s, f, time_us, pin);
    RM_KLAUNCH(k_nbt_count, dim3(kNbtBlocks), dim3(kNbtThreads), 0, s, f, slot);
    RM_KLAUNCH(k_nbt_rest, dim3(relay_blocks(f.n_nodes)), dim3(kNbtThreads), 0, s, f);
    return hipGetLastError();
}

hipError_t launch_nbtable_expire(hipStream_t s, const NbTableDev &f, int64_t time_us, const int32_t *pin)
{
    if (!nbt_dev_ok(f) || time_us < 0) return hipErrorInvalidValue;
    RM_KLAUNCH(k_nbt_expire, dim3(relay_blocks(f.n_nodes)), dim3(kNbtThreads), 0, s, f, time_us, pin);
    return hipGetLastError();
}

} // namespace rm
