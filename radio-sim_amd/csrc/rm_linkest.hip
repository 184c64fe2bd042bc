// rm_linkest.hip -- link estimator: EWMA ETX over counter windows and forwarding acks on the device (DESIGN.md section 6, E23, and
// 4.28) (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// A fold is ONE launch, a lane per entry (j, k): K is 1, 2, 4 or 8, so the K lanes of a row lie inside one wave (64 / K rows per
// wave) and everything a row shares travels by shuffles and one ballot, never through memory:
//   beacon step   the lane's own: the input slot's peer and two counters (16 of the entry's 48 bytes), its rm_linkest_entry (32
//                 bytes), the lest_beacon text of rm_math.hpp
//   data step     the row's lowest lane reads the forwarding row's next / acked / failed and the node state and judges (lest_data);
//                 the verdict and the window go to the row by shuffles; the slot that holds the next hop is the lowest bit of a
//                 ballot cut to the row's lane group, judged on the peers AFTER the beacon step
//   writes        a lane stores its entry only if it changed, the published peer and entry only if etx or peer changed; the row's
//                 lowest lane stores the node state only if it changed.  Nobody reads what another lane of the launch writes.
// The inputs are never written.  Per-node counters need no atomics (one writer); the totals -- one address for everybody -- are
// counted per wave by ballots, summed per workgroup in LDS and added once per workgroup and field (estimates travels as a
// two's-complement delta; one add per WAVE and field was measured first and cost most of the kernel).  All integers:
// nothing depends on launch geometry or on the order in which the atomics land.  192 bytes of LDS, no scratch memory.
#include "rm_device.hpp"

namespace rm {

constexpr int kLestThreads = kRelayThreads;

static int lest_blocks(const LinkEstDev &f)
{
    const long long lanes = (long long)f.n_nodes * (long long)f.K;
    return int(std::max(1ll, (lanes + kLestThreads - 1) / kLestThreads));
}

__global__ void __launch_bounds__(kLestThreads) k_lest_init(const LinkEstDev f)
{
    const long long g = (long long)blockIdx.x * kLestThreads + (long long)threadIdx.x;
    if (g == 0) *f.totals = rm_linkest_totals{};
    if (g < (long long)f.n_nodes) {
        rm_linkest_node nd{};
        nd.base_next = -1;
        f.node[g] = nd;
    }
    if (g >= (long long)f.n_nodes * (long long)f.K) return;
    rm_linkest_entry e{};
    e.peer = -1;
    f.entry[g] = e;
    f.pub_peer[g] = -1;
    rm_link_stats s;
    lest_publish(0u, s);
    f.pub_stats[g] = s;
}

__global__ void __launch_bounds__(kLestThreads) k_lest_fold(const LinkEstDev f)
{
    const long long g = (long long)blockIdx.x * kLestThreads + (long long)threadIdx.x;
    const int lane = int(threadIdx.x) & 63;
    const int K = f.K;                    // (uniform; a power of two that divides 64)
    const int k = lane & (K - 1);
    const int lead = lane - k;            // the row's lowest lane
    const long long jj = g / K;
    const bool live = jj < (long long)f.n_nodes; // (a row is live or not as a whole)
    const int j = live ? int(jj) : 0;
    if (g == 0) atomicAdd(relay_w(&f.totals->folds), 1ull);

    // ---- the beacon step, the lane's own entry
    rm_linkest_entry e{};
    unsigned did = 0u;
    uint32_t etx0 = 0u;
    int32_t peer0 = -1;
    bool e_dirty = false;
    if (live) {
        e = f.entry[g];
        etx0 = e.etx;
        peer0 = e.peer;
        const int32_t p = f.in_peer[g];
        const rm_link_stats *st = f.in_stats + g;
        did = lest_beacon(f.p, f.n_nodes, j, p, st->heard, st->delivered, e);
        // (an untouched empty entry is CLEARED-free and unchanged: nothing to store)
        e_dirty = did != 0u || e.peer != peer0;
    }

    // ---- the data step: the row's lowest lane judges, the row hears by shuffles
    const bool data_on = f.in_fwd != nullptr && f.p.data_window > 0u; // (uniform)
    rm_linkest_node nd{};
    int due = 0;
    int32_t w = -1;
    u64 dT = 0ull, dA = 0ull;
    bool nd_dirty = false;
    if (live && k == 0) {
        nd = f.node[j];
        if (data_on) {
            const rm_fwd_node *fw = f.in_fwd + j;
            const uint64_t A = fw->acked, T = A + fw->failed;
            const rm_linkest_node was = nd;
            uint64_t dt = 0ull, da = 0ull;
            w = fw->next;
            due = lest_data(f.p, f.n_nodes, j, w, T, A, nd, dt, da) ? 1 : 0;
            dT = dt;
            dA = da;
            nd_dirty = was.base_next != nd.base_next || was.base_tx != nd.base_tx || was.base_ack != nd.base_ack;
        }
    }
    // (every lane of the wave takes part in the shuffles and the ballots; all of it is skipped uniformly without a data step)
    int matched = 0, unmatched = 0;
    const u64 group = ((1ull << K) - 1ull) << lead; // the row's lanes (K <= 8)
    if (data_on) {
        due = __shfl(due, lead);
        w = __shfl(w, lead);
        dT = __shfl(dT, lead);
        dA = __shfl(dA, lead);
        const u64 holds = __ballot(live && due && e.peer == w) & group; // (w is a node index other than j: no empty entry equals it)
        if (live && due) {
            if (holds == 0ull) {
                unmatched = k == 0 ? 1 : 0;
            } else if (lane == __ffsll((long long)holds) - 1) {
                lest_data_sample(f.p, dT, dA, e);
                e_dirty = true;
                matched = 1;
            }
        }
    }
    // what the row's lowest lane counts for its node
    const u64 restarts = __ballot(live && (did & LEST_RESTARTED) != 0u) & group;
    const u64 samples = __ballot(matched != 0) & group;

    // ---- the stores
    if (live) {
        if (e_dirty) f.entry[g] = e;
        if (e.etx != etx0 || e.peer != peer0) {
            f.pub_peer[g] = e.peer;
            rm_link_stats s;
            lest_publish(e.etx, s);
            f.pub_stats[g] = s;
        }
        if (k == 0) {
            const uint32_t n_restart = uint32_t(__popcll(restarts)), n_sample = uint32_t(__popcll(samples));
            if (nd_dirty || n_restart || n_sample || unmatched) {
                nd.restarted += n_restart;
                nd.data_samples += n_sample;
                nd.data_unmatched += uint32_t(unmatched);
                f.node[j] = nd;
            }
        }
    }

    // ---- the totals: every count is 0 or 1 per lane, so a wave's share is the population of a ballot; the workgroup's four shares
    // meet in LDS and one lane per field adds the workgroup's sum (beacon_samples .. estimates lie side by side in the struct)
    __shared__ long long s_tot[kLestThreads / 64][6];
    const long long gained = __popcll(__ballot(e.etx != 0u && etx0 == 0u)), lost = __popcll(__ballot(e.etx == 0u && etx0 != 0u));
    const long long share[6] = {(long long)__popcll(__ballot((did & LEST_SAMPLED) != 0u)), (long long)__popcll(__ballot(matched != 0)),
                                (long long)__popcll(__ballot(unmatched != 0)), (long long)__popcll(__ballot((did & LEST_RESTARTED) != 0u)),
                                (long long)__popcll(__ballot((did & LEST_CLEARED) != 0u)), gained - lost};
    if (lane == 0)
        for (int i = 0; i < 6; ++i) s_tot[threadIdx.x >> 6][i] = share[i];
    __syncthreads(); // (no lane has left: every workgroup reaches it whole)
    if (threadIdx.x < 6u) {
        long long sum = 0;
        for (int w = 0; w < kLestThreads / 64; ++w) sum += s_tot[w][threadIdx.x];
        // (estimates may go down: the delta as 64 bits, the sum wraps to the right total)
        if (sum != 0) atomicAdd(relay_w(&f.totals->beacon_samples) + threadIdx.x, u64(sum));
    }
}

// ---- launches

static bool lest_dev_ok(const LinkEstDev &f)
{
    return f.entry && f.node && f.pub_peer && f.pub_stats && f.totals && f.n_nodes >= 1 && (f.K == 1 || f.K == 2 || f.K == 4 || f.K == 8);
}

hipError_t launch_linkest_init(hipStream_t s, const LinkEstDev &f)
{
    if (!lest_dev_ok(f)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_lest_init, dim3(std::max(lest_blocks(f), relay_blocks(f.n_nodes))), dim3(kLestThreads), 0, s, f);
    return hipGetLastError();
}

hipError_t launch_linkest_fold(hipStream_t s, const LinkEstDev &f)
{
    if (!lest_dev_ok(f) || !f.in_peer || !f.in_stats || !lest_valid(f.p)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_lest_fold, dim3(lest_blocks(f)), dim3(kLestThreads), 0, s, f);
    return hipGetLastError();
}

} // namespace rm
