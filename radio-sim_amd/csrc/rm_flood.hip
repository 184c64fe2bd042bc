// rm_flood.hip -- dissemination floods: Trickle-timed broadcast relay on the device
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The table belongs to the context: one 64-byte row per node (rm_flood_node).  Nothing may depend on the order in which atomics
// land, so every call is cut into launches each of which READS only what the launch before it finished and what no lane of its
// own writes:
//   seed      k_flood_seed_claim   atomicMin of the entry's index over claim[j]: one entry per node that lacks the data
//             k_flood_seed_apply   the winners write their node's row; the claim back to rest
//   sources   k_flood_src_count    a node's own lane: due and c >= k -> the suppression roll (and a mark in claim[j]); else counted
//             k_flood_src_scan     the units' counts scanned, the list padded
//             k_flood_src_write    the unmarked due nodes written in ascending order (their state is as at the start); marks cleared
//             (source_walk on both sides of units_scan, rm_device.hpp, with the two bodies above as its membership test)
//   advance   k_flood_adv_claim    atomicMin of p over claim[j]: the first occurrence of every candidate that has the data
//             k_flood_rx_hear      a lane per link: heard[d]++; d with the data and not sending: c[d]++; d without: atomicMin of
//                                  t_end over tmin[d]
//             k_flood_rx_pick      the links at tmin[d]: atomicMin of p over pmin[d]
//             k_flood_settle       the one link with pmin[d] == p writes d's row (receivers of one frame are distinct, so (d, p) is
//                                  one link) and puts d's scratch back to rest; then a lane per packet number: the owner of
//                                  claim[j] decides stray / deferred / sent, writes j's row and puts the claim back to rest
// A node's row is written by plain stores where only one lane can (the seed's winner, the node's own lane in the source walk, the
// winning link, the claim's owner -- rows of nodes WITHOUT the data for the first two writers of an advance, WITH it for the last)
// and by integer atomic adds for heard and c.  A link's packet number is found by a search of the slot's pkt_offset, which
// uc_describe hands out for every slot kind; UcSlot was not given TickDev's out_pkt column, because whether every path that
// materializes a slot's compact arrays also fills that column was not established, and log2(n_new) cached loads per link do not
// depend on it.  The totals -- one address for everybody -- are added once per wave (relay_total, relay_total_max; those, the
// claim step relay_claim and the other relay_* helpers are rm_device.hpp's, shared with the forwarding queues, rm_fwd.hip).  No
// LDS beyond the scan's word, no scratch memory, no floating point.
#include "rm_device.hpp"

namespace rm {

constexpr int kFloodThreads = kRelayThreads;
// Workgroups per pass over the slot's links, as the traffic counters' pass: 16 384 lanes per stride (not tuned)
constexpr int kFloodBlocks = 64;
constexpr int32_t kFloodRest = INT32_MAX;
constexpr long long kFloodNever = INT64_MAX;

RM_D long long *flood_t(int64_t *p) { return reinterpret_cast<long long *>(p); }

RM_D bool flood_due(const FloodDev &f, const rm_flood_node &r, int64_t t)
{
    return r.first_us >= 0 && r.interval < f.max_intervals && r.fire_us <= t;
}

// interval r.interval of node j
RM_D void flood_schedule(const FloodDev &f, rm_flood_node &r, int j)
{
    int64_t start, fire;
    flood_fire(f.imin_us, f.doublings, f.max_intervals, f.seed, j, r.first_us, r.interval, start, fire);
    r.start_us = start;
    r.fire_us = fire;
}

// ---- enable / reset, the tree

__global__ void __launch_bounds__(kFloodThreads) k_flood_init(const FloodDev f)
{
    const int j = int(blockIdx.x) * kFloodThreads + int(threadIdx.x);
    if (j == 0) *f.totals = rm_flood_totals{};
    if (j >= f.n_nodes) return;
    rm_flood_node r{};
    r.first_us = r.start_us = r.fire_us = -1;
    r.parent = r.hop = -1;
    f.node[j] = r;
    f.claim[j] = kFloodRest;
    f.pmin[j] = kFloodRest;
    f.tmin[j] = kFloodNever;
}

__global__ void __launch_bounds__(kFloodThreads) k_flood_tree(const FloodDev f, int32_t *__restrict__ parent, int32_t *__restrict__ hop)
{
    const int j = int(blockIdx.x) * kFloodThreads + int(threadIdx.x);
    if (j >= f.n_nodes) return;
    parent[j] = f.node[j].parent;
    if (hop) hop[j] = f.node[j].hop;
}

// ---- seed

__global__ void __launch_bounds__(kFloodThreads) k_flood_seed_claim(const FloodDev f, const int32_t *__restrict__ nodes, const int n)
{
    const int e = int(blockIdx.x) * kFloodThreads + int(threadIdx.x);
    if (e >= n) return;
    int32_t j = nodes[e];
    if (!relay_in(f, j) || f.node[j].first_us >= 0) j = -1;
    else atomicMin(&f.claim[j], e);
    f.act[e] = j;
}

__global__ void __launch_bounds__(kFloodThreads) k_flood_seed_apply(const FloodDev f, const int n, const int64_t time_us)
{
    const int e = int(blockIdx.x) * kFloodThreads + int(threadIdx.x);
    u64 t_seeds = 0;
    if (e < n) {
        const int32_t j = f.act[e];
        if (j >= 0 && f.claim[j] == e) { // (only the owner puts the claim back: a duplicate reads its owner's index or the rest value)
            f.claim[j] = kFloodRest;
            rm_flood_node &r = f.node[j];
            r.first_us = time_us;
            r.rssi_bits = 0ull;
            r.parent = -1;
            r.hop = 0;
            r.interval = 0;
            r.c = 0;
            flood_schedule(f, r, j);
            t_seeds = 1ull;
        }
    }
    relay_total(&f.totals->seeds, t_seeds);
    relay_total(&f.totals->covered, t_seeds);
    relay_total_max(&f.totals->last_first_us, t_seeds ? u64(time_us) : 0ull);
}

// ---- the source list: the nodes due at time_us that are not suppressed, ascending

// count: a due node with c >= k is suppressed now -- its row moves to the next interval, claim[node] is marked for the write
// launch -- and any other due node is listed
__global__ void __launch_bounds__(64) k_flood_src_count(const FloodDev f, const int64_t time_us, const int chunk, int32_t *unit_count)
{
    u64 t_supp = 0;
    source_walk<false>(f.n_nodes, 0, chunk, unit_count, nullptr, [&](int node) {
        rm_flood_node &r = f.node[node];
        if (!flood_due(f, r, time_us)) return false;
        if (f.redundancy <= 0 || r.c < f.redundancy) return true;
        r.suppressed += 1u;
        r.interval += 1;
        r.c = 0;
        flood_schedule(f, r, node);
        f.claim[node] = -1;
        t_supp += 1ull;
        return false;
    });
    relay_total(&f.totals->suppressed, t_supp);
}

__global__ void __launch_bounds__(256) k_flood_src_scan(const int units, const int cap, int32_t *unit_count, int32_t *out_src, int32_t *out_count)
{
    units_scan(units, 1, cap, unit_count, out_src, out_count);
}

// write: a marked node is not listed and its mark is cleared; the row of any other is as at the start of the call
__global__ void __launch_bounds__(64) k_flood_src_write(const FloodDev f, const int64_t time_us, const int cap, const int chunk, int32_t *unit_count,
                                                        int32_t *out_src)
{
    source_walk<true>(f.n_nodes, cap, chunk, unit_count, out_src, [&](int node) {
        if (f.claim[node] == kFloodRest) return flood_due(f, f.node[node], time_us);
        f.claim[node] = kFloodRest;
        return false;
    });
}

// ---- advance

// (the slot's links and a link's packet: relay_links and relay_pkt of rm_device.hpp, shared with the neighbour tables)
RM_D uint32_t flood_links(const UcSlot &s) { return relay_links(s); }
RM_D int flood_pkt(const UcSlot &s, const uint32_t i) { return relay_pkt(s, i); }

// d, which has the data, transmits in this call: it owns a packet number at which it is due and that the gate let through
RM_D bool flood_sends(const FloodDev &f, const UcSlot &s, const int d)
{
    const int32_t p = f.claim[d];
    if (p < 0 || p == kFloodRest) return false; // (never a mark of the source walk: its write launch clears them)
    return flood_due(f, f.node[d], s.recs[p].start_us) && s.recs[p].src == d;
}

// a delivered link that carries the data: its packet, its two ends and the frame's end
struct FloodLink {
    int p, src, dst;
    int64_t t_end;
};
RM_D bool flood_link(const FloodDev &f, const UcSlot &s, const uint32_t i, FloodLink &l)
{
    if (s.verdict[i] != uint8_t(RM_DELIVERED)) return false;
    l.p = flood_pkt(s, i);
    l.src = s.recs[l.p].src;
    l.dst = s.dst[i];
    if (!relay_in(f, l.src) || !relay_in(f, l.dst)) return false;
    l.t_end = s.recs[l.p].start_us + s.recs[l.p].air_us;
    return true;
}

__global__ void __launch_bounds__(kFloodThreads) k_flood_adv_claim(const FloodDev f, const UcSlot s, const int32_t *__restrict__ cand, const int P)
{
    const int p = int(blockIdx.x) * kFloodThreads + int(threadIdx.x);
    const int32_t j = relay_claim(f, s, cand, P, p, [&](int j) { return f.node[j].first_us >= 0; }); // (a node that has the data)
    if (j != kClaimNone) f.act[p] = j;
}

__global__ void __launch_bounds__(kFloodThreads) k_flood_rx_hear(const FloodDev f, const UcSlot s)
{
    if (relay_slot_lost(s)) return; // (uniform)
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t n = flood_links(s);
    const uint32_t n_up = (n + 63u) & ~63u; // whole waves
    u64 t_heard = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        FloodLink l;
        if (i >= n || !flood_link(f, s, i, l)) continue;
        const rm_flood_node &rs = f.node[l.src];
        if (rs.first_us < 0) continue;
        rm_flood_node &rd = f.node[l.dst];
        atomicAdd(&rd.heard, 1u);
        t_heard += 1ull;
        if (rd.first_us >= 0) {
            if (l.t_end >= rd.start_us && !flood_sends(f, s, l.dst)) atomicAdd(&rd.c, 1);
        } else if (rs.hop + 1 <= f.max_hops) {
            atomicMin(flood_t(&f.tmin[l.dst]), (long long)l.t_end);
        }
    }
    relay_total(&f.totals->heard, t_heard);
}

__global__ void __launch_bounds__(kFloodThreads) k_flood_rx_pick(const FloodDev f, const UcSlot s)
{
    if (relay_slot_lost(s)) return;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t n = flood_links(s);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        FloodLink l;
        if (!flood_link(f, s, i, l)) continue;
        const rm_flood_node &rs = f.node[l.src];
        if (rs.first_us < 0 || f.node[l.dst].first_us >= 0 || rs.hop + 1 > f.max_hops) continue;
        if (f.tmin[l.dst] == l.t_end) atomicMin(&f.pmin[l.dst], l.p);
    }
}

__global__ void __launch_bounds__(kFloodThreads) k_flood_settle(const FloodDev f, const UcSlot s, const int P)
{
    if (relay_slot_lost(s)) return;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t n = flood_links(s);
    const uint32_t n_up = (n + 63u) & ~63u;
    u64 t_new = 0, t_hop = 0, t_last = 0, t_sent = 0, t_deferred = 0, t_stray = 0;
    // the winning links.  Nothing here reads first_us or hop of a node without the data: those are what the winners write
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        FloodLink l;
        if (i >= n || !flood_link(f, s, i, l)) continue;
        if (f.pmin[l.dst] != l.p) continue; // (at rest for every node that had the data or no candidate link; p < n_new < the rest value)
        f.pmin[l.dst] = kFloodRest;
        f.tmin[l.dst] = kFloodNever;
        rm_flood_node &r = f.node[l.dst];
        r.first_us = l.t_end;
        r.rssi_bits = s.rssi ? reinterpret_cast<const uint64_t *>(s.rssi)[i] : 0ull;
        r.parent = l.src;
        r.hop = f.node[l.src].hop + 1;
        r.interval = 0;
        r.c = 0;
        flood_schedule(f, r, l.dst);
        t_new += 1ull;
        t_hop = max(t_hop, u64(r.hop));
        t_last = max(t_last, u64(l.t_end > 0 ? l.t_end : 0));
    }
    // the transmitters: rows of nodes WITH the data, which no winner above writes
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < uint32_t(P); p += stride) {
        const int32_t j = f.act[p];
        if (j < 0) continue;
        if (f.claim[j] != int32_t(p)) { // a later occurrence (it reads the owner's number or the rest value)
            t_stray += 1ull;
            continue;
        }
        f.claim[j] = kFloodRest;
        rm_flood_node &r = f.node[j];
        if (!flood_due(f, r, s.recs[p].start_us)) {
            t_stray += 1ull;
        } else if (s.recs[p].src != j) {
            r.deferred += 1u;
            t_deferred += 1ull;
        } else {
            r.sent += 1u;
            r.interval += 1;
            r.c = 0;
            flood_schedule(f, r, j);
            t_sent += 1ull;
        }
    }
    relay_total(&f.totals->covered, t_new);
    relay_total(&f.totals->sent, t_sent);
    relay_total(&f.totals->deferred, t_deferred);
    relay_total(&f.totals->stray, t_stray);
    relay_total_max(&f.totals->max_hop, t_hop);
    relay_total_max(&f.totals->last_first_us, t_last);
}

// ---- launches

static bool flood_dev_ok(const FloodDev &f)
{
    return f.node && f.totals && f.claim && f.pmin && f.tmin && f.n_nodes >= 0 && f.max_intervals >= 1 && f.max_intervals <= 64 && f.imin_us >= 2;
}

hipError_t launch_flood_init(hipStream_t s, const FloodDev &f)
{
    if (!flood_dev_ok(f)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_flood_init, dim3(relay_blocks(f.n_nodes)), dim3(kFloodThreads), 0, s, f);
    return hipGetLastError();
}

hipError_t launch_flood_tree(hipStream_t s, const FloodDev &f, int32_t *parent, int32_t *hop)
{
    if (!flood_dev_ok(f) || !parent) return hipErrorInvalidValue;
    RM_KLAUNCH(k_flood_tree, dim3(relay_blocks(f.n_nodes)), dim3(kFloodThreads), 0, s, f, parent, hop);
    return hipGetLastError();
}

hipError_t launch_flood_seed(hipStream_t s, const FloodDev &f, const int32_t *nodes, int n, int64_t time_us)
{
    if (n <= 0) return hipSuccess;
    if (!flood_dev_ok(f) || !nodes || !f.act) return hipErrorInvalidValue;
    RM_KLAUNCH(k_flood_seed_claim, dim3(relay_blocks(n)), dim3(kFloodThreads), 0, s, f, nodes, n);
    RM_KLAUNCH(k_flood_seed_apply, dim3(relay_blocks(n)), dim3(kFloodThreads), 0, s, f, n, time_us);
    return hipGetLastError();
}

hipError_t launch_flood_sources(hipStream_t s, const FloodDev &f, int64_t time_us, int cap, int units, int chunk, int32_t *unit_count,
                                int32_t *out_src, int32_t *out_count)
{
    if (!flood_dev_ok(f) || cap < 1 || units < 1 || chunk < 64 || !unit_count || !out_src || !out_count) return hipErrorInvalidValue;
    if (int64_t(units) * chunk < f.n_nodes) return hipErrorInvalidValue;
    RM_KLAUNCH(k_flood_src_count, dim3(units), dim3(64), 0, s, f, time_us, chunk, unit_count);
    RM_KLAUNCH(k_flood_src_scan, dim3(1), dim3(256), 0, s, units, cap, unit_count, out_src, out_count);
    RM_KLAUNCH(k_flood_src_write, dim3(units), dim3(64), 0, s, f, time_us, cap, chunk, unit_count, out_src);
    return hipGetLastError();
}

hipError_t launch_flood_advance(hipStream_t s, const FloodDev &f, const UcSlot &slot, const int32_t *cand, int P)
{
    if (!flood_dev_ok(f) || P < 0 || P > slot.n_new || (P > 0 && (!f.act || !slot.recs))) return hipErrorInvalidValue;
    RM_KLAUNCH(k_flood_adv_claim, dim3(relay_blocks(P)), dim3(kFloodThreads), 0, s, f, slot, cand, P); // (also with P == 0: a lost slot is counted)
    if (slot.n_new <= 0) return hipGetLastError();
    RM_KLAUNCH(k_flood_rx_hear, dim3(kFloodBlocks), dim3(kFloodThreads), 0, s, f, slot);
    RM_KLAUNCH(k_flood_rx_pick, dim3(kFloodBlocks), dim3(kFloodThreads), 0, s, f, slot);
    RM_KLAUNCH(k_flood_settle, dim3(kFloodBlocks), dim3(kFloodThreads), 0, s, f, slot, P);
    return hipGetLastError();
}

} // namespace rm
