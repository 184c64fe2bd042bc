// rm_traffic.hip -- traffic schedules: periodic sources generated on the device
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The generator turns the context's table of {period_us, phase_us, jitter_us} records, for a batch of time windows, into one
// source list per window: the nodes with a packet due inside it, in ascending node index -- an ORDERED stream compaction into up
// to RM_MAX_BATCH rows at once.  The node table is cut into units of `chunk` consecutive nodes, one wave (one 64-thread workgroup)
// per unit, one lane per node, 64 nodes a round:
//   k_traffic_count  every unit's sources per window (unit_count [units][n_ticks]) and its packets (unit_packets [units])
//   k_traffic_scan   one workgroup per window: its column becomes exclusive prefixes over the units, count[b] is the column's sum,
//                    and the row's tail behind min(count[b], cap) is padded with -1
//   k_traffic_write  the walk again; a lane writes its node at the unit's prefix + the sources before it in the unit
//                    (clipped at cap); unit 0 sums the totals
// The walk of a node is traffic_before (rm_math.hpp) at the windows' edges, carried forward: n = the packets due before the time
// reached so far.  A node without a packet in the batch's span leaves after the two calls at the span's ends -- at most two 64-bit
// divisions -- and a round in which no lane has one skips the window loop.  Inside the loop an edge at or before the next
// packet's interval is one comparison, one within a period behind it needs no division, and only a packet whose jitter interval
// contains the edge is hashed: the work of a node follows its windows, never its packets.  The windows are read at wave-uniform
// addresses.  Integer arithmetic only; no atomics, so nothing depends on the order in which units run.
#include "rm_device.hpp"

namespace rm {

bool host_traffic_valid(const rm_traffic_schedule &s) { return traffic_valid(s); }
int64_t host_traffic_due(const rm_traffic_schedule &s, uint64_t seed, int32_t node, int64_t k) { return traffic_due(s, seed, node, k); }

// Units at most (not tuned): unit_count is units * n_ticks words, 4 MiB at 512 windows.
constexpr int kTrafficUnits = 2048;

void traffic_geometry(int n_nodes, int *units, int *chunk)
{
    const int rounds = (std::max(n_nodes, 1) + 63) / 64;
    const int per = (rounds + kTrafficUnits - 1) / kTrafficUnits; // rounds of 64 nodes per unit
    *chunk = per * 64;
    *units = (rounds + per - 1) / per;
}

// s_run[b]: COUNT -- the unit's sources of window b so far; WRITE -- where its next source of window b goes.  Lane 0 alone reads
// and writes it inside the rounds.
template <bool WRITE> RM_D void traffic_walk(const TrafficGen &g, int32_t *s_run)
{
    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int W = g.n_ticks;
    for (int b = lane; b < W; b += 64) s_run[b] = WRITE ? g.unit_count[size_t(unit) * W + b] : 0;
    __syncthreads();
    const int64_t span_lo = g.win[0], span_hi = g.win[2 * W - 1];
    const int first = unit * g.chunk;
    const int last = min(first + g.chunk, g.n_nodes);
    uint64_t packets = 0;
    for (int i0 = first; i0 < last; i0 += 64) {
        const int node = i0 + lane;
        rm_traffic_schedule sc{};
        if (node < last) sc = g.sched[node];
        int64_t n = 0, n_end = 0; // packets due before the time reached / before the span's end
        if (sc.period_us > 0) {
            n = traffic_before(sc, g.seed, node, span_lo, 0);
            n_end = traffic_before(sc, g.seed, node, span_hi, n);
        }
        for (int b = 0; b < W; ++b) {
            if (ballot64(n != n_end) == 0ull) break; // nobody of this round has a packet left in the span
            const int64_t lo = g.win[b], hi = g.win[W + b];
            bool hit = false;
            if (n != n_end) {
                const int64_t a = traffic_before(sc, g.seed, node, lo, n);
                n = traffic_before(sc, g.seed, node, hi, a);
                hit = n != a;
                if (!WRITE) packets += uint64_t(n - a);
            }
            const uint64_t m = ballot64(hit);
            if (m == 0ull) continue;
            if (WRITE) {
                int base = 0;
                if (lane == 0) {
                    base = s_run[b];
                    s_run[b] = base + __popcll(m);
                }
                const int pos = uniform_i(base) + int(lane_prefix(m));
                if (hit && pos < g.cap) g.out_src[size_t(b) * size_t(g.cap) + size_t(pos)] = node;
            } else if (lane == 0) {
                s_run[b] += __popcll(m);
            }
        }
    }
    if (!WRITE) {
        __syncthreads();
        for (int b = lane; b < W; b += 64) g.unit_count[size_t(unit) * W + b] = s_run[b];
        packets = wave_sum_u64(packets);
        if (lane == 0) g.unit_packets[unit] = packets;
    }
}

__global__ void __launch_bounds__(64) k_traffic_count(const TrafficGen g)
{
    __shared__ int32_t s_run[kMaxBatch];
    traffic_walk<false>(g, s_run);
}

__global__ void __launch_bounds__(64) k_traffic_write(const TrafficGen g)
{
    __shared__ int32_t s_run[kMaxBatch];
    traffic_walk<true>(g, s_run);
    if (blockIdx.x != 0 || !g.out_totals) return;
    // the totals: integer sums, any order
    const int lane = threadIdx.x;
    unsigned long long packets = 0, pairs = 0, truncated = 0;
    for (int u = lane; u < g.units; u += 64) packets += g.unit_packets[u];
    for (int b = lane; b < g.n_ticks; b += 64) {
        const int32_t c = g.out_count[b];
        pairs += uint64_t(c);
        if (c > g.cap) truncated += uint64_t(c - g.cap);
    }
    packets = wave_sum_u64(packets);
    pairs = wave_sum_u64(pairs);
    truncated = wave_sum_u64(truncated);
    if (lane == 0) {
        g.out_totals->packets = packets;
        g.out_totals->coalesced = packets - pairs;
        g.out_totals->truncated = truncated;
    }
}

// window blockIdx.x: its column of unit_count and its row of out_src (units_scan, rm_device.hpp)
__global__ void __launch_bounds__(256) k_traffic_scan(const TrafficGen g)
{
    const int b = blockIdx.x;
    units_scan(g.units, g.n_ticks, g.cap, g.unit_count + b, g.out_src + size_t(b) * size_t(g.cap), g.out_count + b);
}

hipError_t launch_traffic_generate(hipStream_t s, const TrafficGen &g)
{
    if (g.n_ticks < 1 || g.n_ticks > kMaxBatch || g.cap < 1 || g.units < 1 || g.chunk < 64 || g.n_nodes < 0) return hipErrorInvalidValue;
    if (int64_t(g.units) * g.chunk < g.n_nodes) return hipErrorInvalidValue;
    RM_KLAUNCH(k_traffic_count, dim3(g.units), dim3(64), 0, s, g);
    RM_KLAUNCH(k_traffic_scan, dim3(g.n_ticks), dim3(256), 0, s, g);
    RM_KLAUNCH(k_traffic_write, dim3(g.units), dim3(64), 0, s, g);
    return hipGetLastError();
}

} // namespace rm
