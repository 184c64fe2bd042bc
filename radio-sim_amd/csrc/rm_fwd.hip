// rm_fwd.hip -- forwarding queues: multi-hop packet relay on the device
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The tables belong to the context: one 128-byte row per node (rm_fwd_node: counters, next, tries, ready_us, the occupancy mask of
// its slots) and queue_slots packets per node.  A queue is a SET of occupied slots; its order is the packets' own
// (enq_us, birth_us, origin, hops), found by a walk over at most 16 slots, so no kernel ever moves a packet.
//
// Nothing may depend on the order in which atomics land.  Every call that pushes is therefore cut into launches with a lane per
// packet number, each of which READS only what the launch before it finished and what no lane of its own writes:
//   advance   k_fwd_adv_claim   atomicMin of p over claim[j]: the first occurrence of every candidate
//             k_fwd_adv_match   the winners: sendable at the frame's start? -> the case of the attempt (the unicast query's search,
//                               rm_device.hpp), A[w] counted for the delivered ones at a relay
//             k_fwd_adv_accept  len_start[w] + A[w] <= Q: the accepted take the k-th slot that was free at the start of the call
//                               (k: an atomic ticket -- WHICH packet lands in which slot is not observable) and write their packet
//             k_fwd_adv_apply   pops, masks, lengths, counters, tries and ready_us; the scratch of the participants back to rest
//   inject    k_fwd_inj_place   tickets per node, the packets written;  k_fwd_inj_apply  masks, lengths, counters
// Rows are written with integer atomics where another lane may write the same word (commutative: add, or, and, max) and with
// plain stores where only the node's own lane can (a node participates once per call).  The totals -- one address for everybody --
// are added once per wave (relay_total).  The source list is an ordered stream compaction, k_fwd_src_count / _scan / _write:
// source_walk with fwd_sendable as the membership test on both sides of units_scan.  Those, relay_claim and the small relay_*
// helpers are rm_device.hpp's, shared with the floods (rm_flood.hip); the queue order is rm_math.hpp's fwd_packet_order.  No LDS
// beyond the scan's word, no scratch memory, no floating point.
#include "rm_device.hpp"

namespace rm {

constexpr int kFwdThreads = kRelayThreads;
enum { kFwdNone = 0, kFwdStray, kFwdDeferred, kFwdFailed, kFwdRejected, kFwdPending, kFwdSink, kFwdPush, kFwdTtl, kFwdNoRoute, kFwdFull };

// the slot of node j's head (-1: the queue is empty) and the head itself
RM_D int fwd_head(const FwdDev &f, int j, uint32_t mask, rm_fwd_packet &head)
{
    int at = -1;
    mask &= (1u << f.Q) - 1u;
    while (mask) {
        const int s = __ffs(int(mask)) - 1;
        mask &= mask - 1u;
        const rm_fwd_packet q = f.pk[size_t(j) * size_t(f.Q) + size_t(s)];
        if (at < 0 || fwd_packet_order(q, head)) {
            head = q;
            at = s;
        }
    }
    return at;
}

RM_D bool fwd_sendable(const FwdDev &f, int j, int64_t t, int *head_slot)
{
    const rm_fwd_node &r = f.node[j];
    rm_fwd_packet head{};
    const int at = fwd_head(f, j, r.slot_mask, head);
    if (head_slot) *head_slot = at;
    return at >= 0 && r.ready_us <= t && head.enq_us <= t;
}

// the k-th slot (k = 0 ..) that `mask` leaves free, -1: there is none
RM_D int fwd_free_slot(const FwdDev &f, uint32_t mask, int k)
{
    uint32_t free = ~mask & ((1u << f.Q) - 1u);
    for (int i = 0; i < k && free; ++i) free &= free - 1u;
    return free ? __ffs(int(free)) - 1 : -1;
}

// a packet that arrives at a sink at time t with `hops` hops behind it
RM_D void fwd_arrive(const FwdDev &f, const rm_fwd_packet &q, int64_t t, int hops, u64 &t_arrived, u64 &t_lat, u64 &t_hops)
{
    const u64 lat = u64(t - q.birth_us);
    if (relay_in(f, q.origin)) {
        rm_fwd_node &o = f.node[q.origin];
        atomicAdd(relay_w(&o.arrived), 1ull);
        atomicAdd(relay_w(&o.latency_us_sum), lat);
        atomicMax(relay_w(&o.latency_us_max), lat);
        atomicAdd(relay_w(&o.hops_sum), u64(hops));
    }
    t_arrived += 1ull, t_lat += lat, t_hops += u64(hops);
}

// a packet dropped at node `at`
RM_D void fwd_drop(const FwdDev &f, const rm_fwd_packet &q, int at)
{
    if (relay_in(f, q.origin)) atomicAdd(relay_w(&f.node[q.origin].lost), 1ull);
    atomicAdd(relay_w(&f.node[at].dropped), 1ull);
}

// ---- enable / reset, routes

__global__ void __launch_bounds__(kFwdThreads) k_fwd_init(const FwdDev f, const int keep_next)
{
    const int j = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (j == 0) *f.totals = rm_fwd_totals{};
    if (j >= f.n_nodes) return;
    rm_fwd_node r{};
    r.next = keep_next ? f.node[j].next : RM_FWD_NO_ROUTE;
    f.node[j] = r;
    f.claim[j] = INT32_MAX;
    f.acc[j] = 0;
    f.pushed[j] = 0;
}

__global__ void __launch_bounds__(kFwdThreads) k_fwd_next(const FwdDev f, const int32_t *__restrict__ parent)
{
    const int j = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (j >= f.n_nodes) return;
    const int32_t v = parent[j];
    f.node[j].next = (relay_in(f, v) && v != j) ? v : RM_FWD_NO_ROUTE;
}

__global__ void __launch_bounds__(kFwdThreads) k_fwd_roots(const FwdDev f, const int32_t *__restrict__ roots, const int n_roots)
{
    const int k = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (k >= n_roots) return;
    const int32_t r = roots[k];
    if (relay_in(f, r)) f.node[r].next = RM_FWD_SINK; // (duplicates store the same value)
}

// the queues of the nodes that are now sinks or without a route
__global__ void __launch_bounds__(kFwdThreads) k_fwd_settle(const FwdDev f, const int64_t time_us)
{
    const int j = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    u64 t_arrived = 0, t_lat = 0, t_hops = 0, t_noroute = 0, t_gone = 0;
    if (j < f.n_nodes) {
        rm_fwd_node &r = f.node[j];
        const int32_t nx = r.next;
        if (nx < 0) {
            r.tries = 0;
            uint32_t mask = r.slot_mask & ((1u << f.Q) - 1u);
            while (mask) {
                const int s = __ffs(int(mask)) - 1;
                mask &= mask - 1u;
                const rm_fwd_packet q = f.pk[size_t(j) * size_t(f.Q) + size_t(s)];
                if (nx == RM_FWD_SINK) {
                    fwd_arrive(f, q, time_us, q.hops, t_arrived, t_lat, t_hops);
                } else {
                    fwd_drop(f, q, j);
                    t_noroute += 1ull;
                }
                t_gone += 1ull;
            }
            r.slot_mask = 0u; // (nobody else writes this row's queue here: pushes are other calls)
            r.queue_len = 0;
        }
    }
    relay_total(&f.totals->arrived, t_arrived);
    relay_total(&f.totals->latency_us_sum, t_lat);
    relay_total(&f.totals->hops_sum, t_hops);
    relay_total(&f.totals->dropped_no_route, t_noroute);
    relay_total(&f.totals->in_flight, 0ull - t_gone);
}

// ---- inject

__global__ void __launch_bounds__(kFwdThreads) k_fwd_inj_place(const FwdDev f, const int32_t *__restrict__ src, const int n, const int64_t time_us)
{
    const int e = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (e >= n) return;
    FwdAct a{};
    a.j = a.w = a.head = a.push = -1;
    const int32_t j = src[e];
    if (relay_in(f, j)) {
        a.j = j;
        const rm_fwd_node &r = f.node[j];
        if (r.next == RM_FWD_SINK) {
            a.state = kFwdSink;
        } else if (r.next < 0) {
            a.state = kFwdNoRoute;
        } else {
            const int k = atomicAdd(&f.pushed[j], 1);
            const int slot = (r.queue_len + k < f.Q) ? fwd_free_slot(f, r.slot_mask, k) : -1;
            a.state = kFwdFull;
            if (slot >= 0) {
                f.pk[size_t(j) * size_t(f.Q) + size_t(slot)] = rm_fwd_packet{j, 0, time_us, time_us};
                a.state = kFwdPush;
                a.push = slot;
                a.qmax = r.queue_len + k + 1;
            }
        }
    }
    f.act[e] = a;
}

__global__ void __launch_bounds__(kFwdThreads) k_fwd_inj_apply(const FwdDev f, const int n)
{
    const int e = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    u64 t_gen = 0, t_arrived = 0, t_noroute = 0, t_full = 0, t_in = 0;
    if (e < n) {
        const FwdAct a = f.act[e];
        if (a.j >= 0) {
            rm_fwd_node &r = f.node[a.j];
            atomicAdd(relay_w(&r.generated), 1ull);
            t_gen = 1ull;
            if (a.state == kFwdSink) {
                atomicAdd(relay_w(&r.arrived), 1ull);
                t_arrived = 1ull;
            } else if (a.state == kFwdPush) {
                atomicOr(&r.slot_mask, 1u << a.push);
                atomicAdd(&r.queue_len, 1);
                atomicMax(&r.queue_max, a.qmax);
                t_in = 1ull;
            } else {
                atomicAdd(relay_w(&r.lost), 1ull);
                atomicAdd(relay_w(&r.dropped), 1ull);
                if (a.state == kFwdNoRoute) t_noroute = 1ull;
                else t_full = 1ull;
            }
            f.pushed[a.j] = 0;
        }
    }
    relay_total(&f.totals->generated, t_gen);
    relay_total(&f.totals->arrived, t_arrived);
    relay_total(&f.totals->dropped_no_route, t_noroute);
    relay_total(&f.totals->dropped_full, t_full);
    relay_total(&f.totals->in_flight, t_in);
}

// ---- the source list: the nodes sendable at time_us, ascending

__global__ void __launch_bounds__(64) k_fwd_src_count(const FwdDev f, const int64_t time_us, const int chunk, int32_t *unit_count)
{
    source_walk<false>(f.n_nodes, 0, chunk, unit_count, nullptr, [&](int node) { return fwd_sendable(f, node, time_us, nullptr); });
}

__global__ void __launch_bounds__(256) k_fwd_src_scan(const int units, const int cap, int32_t *unit_count, int32_t *out_src, int32_t *out_count)
{
    units_scan(units, 1, cap, unit_count, out_src, out_count);
}

__global__ void __launch_bounds__(64) k_fwd_src_write(const FwdDev f, const int64_t time_us, const int cap, const int chunk, int32_t *unit_count,
                                                      int32_t *out_src)
{
    source_walk<true>(f.n_nodes, cap, chunk, unit_count, out_src, [&](int node) { return fwd_sendable(f, node, time_us, nullptr); });
}

// ---- advance

__global__ void __launch_bounds__(kFwdThreads) k_fwd_adv_claim(const FwdDev f, const UcSlot s, const int32_t *__restrict__ cand, const int P)
{
    const int p = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    const int32_t j = relay_claim(f, s, cand, P, p, [](int) { return true; }); // (every node of the table takes part)
    if (j != kClaimNone) f.act[p].j = j;
}

__global__ void __launch_bounds__(kFwdThreads) k_fwd_adv_match(const FwdDev f, const UcSlot s, const int P)
{
    const int p = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (p >= P || relay_slot_lost(s)) return;
    FwdAct a{};
    a.j = f.act[p].j;
    a.w = a.head = a.push = -1;
    if (a.j >= 0) {
        a.state = kFwdStray;
        if (f.claim[a.j] == p && fwd_sendable(f, a.j, s.recs[p].start_us, &a.head)) {
            const int32_t w = f.node[a.j].next;
            a.state = kFwdFailed;
            if (relay_in(f, w)) { // (a non-empty queue implies it)
                a.w = w;
                int32_t link;
                if (s.recs[p].src != a.j) {
                    a.state = kFwdDeferred;
                } else if (uc_find(s, p, w, f.n_nodes, link) == RM_UC_DELIVERED) {
                    if (f.node[w].next == RM_FWD_SINK) {
                        a.state = kFwdSink;
                    } else {
                        a.state = kFwdPending;
                        atomicAdd(&f.acc[w], 1);
                    }
                }
            }
        }
    }
    f.act[p] = a;
}

__global__ void __launch_bounds__(kFwdThreads) k_fwd_adv_accept(const FwdDev f, const UcSlot s, const int P)
{
    const int p = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (p >= P || relay_slot_lost(s)) return;
    FwdAct a = f.act[p];
    if (a.state != kFwdPending) return;
    const rm_fwd_node &w = f.node[a.w];
    a.state = kFwdRejected;
    if (w.queue_len + f.acc[a.w] <= f.Q) {
        const rm_fwd_packet q = f.pk[size_t(a.j) * size_t(f.Q) + size_t(a.head)];
        if (q.hops + 1 > f.max_hops) {
            a.state = kFwdTtl;
        } else {
            const int k = atomicAdd(&f.pushed[a.w], 1);
            const int slot = fwd_free_slot(f, w.slot_mask, k);
            if (slot >= 0) { // (there is one: len_start + A <= Q)
                f.pk[size_t(a.w) * size_t(f.Q) + size_t(slot)] = rm_fwd_packet{q.origin, q.hops + 1, q.birth_us, s.recs[p].start_us + s.recs[p].air_us};
                a.state = kFwdPush;
                a.push = slot;
                a.qmax = w.queue_len + k + 1;
            }
        }
    }
    f.act[p] = a;
}

__global__ void __launch_bounds__(kFwdThreads) k_fwd_adv_apply(const FwdDev f, const UcSlot s, const int P)
{
    const int p = int(blockIdx.x) * kFwdThreads + int(threadIdx.x);
    if (relay_slot_lost(s)) return; // (uniform)
    u64 t_arrived = 0, t_lat = 0, t_hops = 0, t_retries = 0, t_ttl = 0, t_stray = 0, t_in = 0;
    if (p < P) {
        const FwdAct a = f.act[p];
        if (a.j >= 0) f.claim[a.j] = INT32_MAX; // (every occurrence stores the same value)
        if (a.state == kFwdStray) t_stray = 1ull;
        if (a.state >= kFwdDeferred) {
            rm_fwd_node &r = f.node[a.j];
            const int64_t start = s.recs[p].start_us, t_end = start + s.recs[p].air_us;
            if (a.w >= 0) f.acc[a.w] = 0, f.pushed[a.w] = 0;
            r.attempts += 1;
            const rm_fwd_packet q = f.pk[size_t(a.j) * size_t(f.Q) + size_t(a.head)];
            bool pop = false;
            if (a.state == kFwdSink || a.state == kFwdPush || a.state == kFwdTtl) {
                pop = true;
                r.acked += 1;
                r.tries = 0;
                r.ready_us = t_end;
                if (a.state == kFwdSink) {
                    fwd_arrive(f, q, t_end, q.hops + 1, t_arrived, t_lat, t_hops);
                } else if (a.state == kFwdTtl) {
                    fwd_drop(f, q, a.w);
                    t_ttl = 1ull;
                } else {
                    rm_fwd_node &w = f.node[a.w];
                    atomicOr(&w.slot_mask, 1u << a.push);
                    atomicAdd(&w.queue_len, 1);
                    atomicMax(&w.queue_max, a.qmax);
                    t_in += 1ull;
                }
            } else {
                if (a.state == kFwdDeferred) r.deferred += 1;
                else r.failed += 1;
                if (a.state == kFwdRejected) atomicAdd(relay_w(&f.node[a.w].rejected), 1ull);
                const int tries = r.tries + 1;
                if (tries > f.max_retries) {
                    pop = true;
                    fwd_drop(f, q, a.j);
                    t_retries = 1ull;
                    r.tries = 0;
                    r.ready_us = t_end;
                } else {
                    r.tries = tries;
                    r.ready_us = t_end + int64_t(fwd_backoff_factor(f.seed, f.min_be, f.max_be, a.j, start, tries)) * f.unit_us;
                }
            }
            if (pop) {
                atomicAnd(&r.slot_mask, ~(1u << a.head));
                atomicSub(&r.queue_len, 1);
                t_in -= 1ull;
            }
        }
    }
    relay_total(&f.totals->arrived, t_arrived);
    relay_total(&f.totals->latency_us_sum, t_lat);
    relay_total(&f.totals->hops_sum, t_hops);
    relay_total(&f.totals->dropped_retries, t_retries);
    relay_total(&f.totals->dropped_ttl, t_ttl);
    relay_total(&f.totals->stray, t_stray);
    relay_total(&f.totals->in_flight, t_in);
}

// ---- launches

static bool fwd_dev_ok(const FwdDev &f)
{
    return f.node && f.pk && f.totals && f.claim && f.acc && f.pushed && f.n_nodes >= 0 && f.Q >= 1 && f.Q <= 16;
}

hipError_t launch_fwd_init(hipStream_t s, const FwdDev &f, bool keep_next)
{
    if (!fwd_dev_ok(f)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_fwd_init, dim3(relay_blocks(f.n_nodes)), dim3(kFwdThreads), 0, s, f, keep_next ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_fwd_set_next(hipStream_t s, const FwdDev &f, const int32_t *parent, const int32_t *roots, int n_roots, int64_t time_us)
{
    if (!fwd_dev_ok(f) || !parent || n_roots < 0 || (n_roots > 0 && !roots)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_fwd_next, dim3(relay_blocks(f.n_nodes)), dim3(kFwdThreads), 0, s, f, parent);
    if (n_roots > 0) RM_KLAUNCH(k_fwd_roots, dim3(relay_blocks(n_roots)), dim3(kFwdThreads), 0, s, f, roots, n_roots);
    RM_KLAUNCH(k_fwd_settle, dim3(relay_blocks(f.n_nodes)), dim3(kFwdThreads), 0, s, f, time_us);
    return hipGetLastError();
}

hipError_t launch_fwd_inject(hipStream_t s, const FwdDev &f, const int32_t *src, int n, int64_t time_us)
{
    if (n <= 0) return hipSuccess;
    if (!fwd_dev_ok(f) || !src || !f.act) return hipErrorInvalidValue;
    RM_KLAUNCH(k_fwd_inj_place, dim3(relay_blocks(n)), dim3(kFwdThreads), 0, s, f, src, n, time_us);
    RM_KLAUNCH(k_fwd_inj_apply, dim3(relay_blocks(n)), dim3(kFwdThreads), 0, s, f, n);
    return hipGetLastError();
}

hipError_t launch_fwd_sources(hipStream_t s, const FwdDev &f, int64_t time_us, int cap, int units, int chunk, int32_t *unit_count, int32_t *out_src,
                              int32_t *out_count)
{
    if (!fwd_dev_ok(f) || cap < 1 || units < 1 || chunk < 64 || !unit_count || !out_src || !out_count) return hipErrorInvalidValue;
    if (int64_t(units) * chunk < f.n_nodes) return hipErrorInvalidValue;
    RM_KLAUNCH(k_fwd_src_count, dim3(units), dim3(64), 0, s, f, time_us, chunk, unit_count);
    RM_KLAUNCH(k_fwd_src_scan, dim3(1), dim3(256), 0, s, units, cap, unit_count, out_src, out_count);
    RM_KLAUNCH(k_fwd_src_write, dim3(units), dim3(64), 0, s, f, time_us, cap, chunk, unit_count, out_src);
    return hipGetLastError();
}

hipError_t launch_fwd_advance(hipStream_t s, const FwdDev &f, const UcSlot &slot, const int32_t *cand, int P)
{
    if (!fwd_dev_ok(f) || P < 0 || P > slot.n_new || (P > 0 && (!f.act || !slot.recs))) return hipErrorInvalidValue;
    const dim3 grid(relay_blocks(P)), block(kFwdThreads);
    RM_KLAUNCH(k_fwd_adv_claim, grid, block, 0, s, f, slot, cand, P); // (also with P == 0: a lost slot is counted)
    if (P == 0) return hipGetLastError();
    RM_KLAUNCH(k_fwd_adv_match, grid, block, 0, s, f, slot, P);
    RM_KLAUNCH(k_fwd_adv_accept, grid, block, 0, s, f, slot, P);
    RM_KLAUNCH(k_fwd_adv_apply, grid, block, 0, s, f, slot, P);
    return hipGetLastError();
}

} // namespace rm
