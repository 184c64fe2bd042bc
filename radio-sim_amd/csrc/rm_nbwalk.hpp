// rm_nbwalk.hpp -- what the queries over the potential-link graph share: the neighbour query (rm_neighbors.hip; DESIGN.md section
// 6, E16), the hop query (rm_hops.hip; E17) and the route query (rm_routes.hip; E18).  The rule's order and the txpower key of
// k_nb_prep; nb_walk, the walk over one node's potential links as a device template that takes the per-round visitor; and what
// the two tree queries have as one text -- nb_seed (the roots claimed into frontier 0), NbBest (a lane's and then a wave's best
// link by the rule's order, the parent passes) -- and RM_NB_BY_DIR_SCAN, the launch of a kernel that is a template of the
// direction and the scan.
// nb_walk has the pair tests and arithmetic, the box / group / receiver walk and the whole-table scan of k_nb_query.  k_nb_query
// keeps its own inlined copy of the walk, and nb_absorb its own butterfly, because taking the template there moved its HEARS box
// variant from 45 to 47 VGPRs.  A change to the walk has to be made in both places: the hop query's tests hold
// the two to each other (tests/test_gpu_hops.py, the 65 537-node case) and both to the oracle.
// Device code only; gfx950, wave64.
#pragma once

#include "rm_device.hpp"

namespace rm {

constexpr int kNbWaves = kWavesPerBlock; // queried entries per workgroup: one wave each
constexpr uint64_t kNbNoRssi = 0x7FF8000000000000ull;

// a txpower as a word whose unsigned order is the values' order (for the one atomicMax of k_nb_prep; it bounds a cut-off, so the
// two zeros may differ): 0 for a NaN, which no number maps to -- and back, 0 giving -inf: nobody is in reach
RM_D unsigned long long nb_value_key(const double v)
{
    if (v != v) return 0ull;
    const uint64_t b = f2u(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
RM_D double nb_key_value(const unsigned long long key)
{
    if (key == 0ull) return -__builtin_inf();
    return u2f((key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key);
}

// THE order of the rule: link a precedes link b
RM_D bool nb_precedes(const double ra, const int na, const double rb, const int nb) { return ra > rb || (ra == rb && na < nb); }

// The best link seen so far by the rule's order, with one 32-bit word that travels with it (a link cost; a kernel that has none
// passes 0 and WORD = false to `wave`, and the word costs nothing).
struct NbBest {
    double rssi = 0.0;
    int node = -1;
    uint32_t word = 0u;
    bool valid = false;
    // a lane's own candidate
    __device__ __forceinline__ void offer(const double r, const int n, const uint32_t w)
    {
        if (!valid || nb_precedes(r, n, rssi, node)) {
            rssi = r;
            node = n;
            word = w;
            valid = true;
        }
    }
    // the wave-wide best in every lane: a butterfly of six exchanges, called by the whole wave
    template <bool WORD> __device__ __forceinline__ void wave()
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double o_r = __shfl_xor(rssi, d);
            const int o_n = __shfl_xor(node, d);
            const uint32_t o_w = WORD ? uint32_t(__shfl_xor(int(word), d)) : 0u;
            const bool o_v = __shfl_xor(int(valid), d) != 0;
            if (o_v) offer(o_r, o_n, o_w);
        }
    }
};

// The roots of a tree query: an entry inside the table that claim(node) wins -- a root listed twice is claimed once -- goes into
// queue[0 .. *tail), frontier 0; *tail is zero in front of the launch.  An entry outside the table is skipped.  The loop is
// workgroup-uniform, so that whole waves reach the append.
template <typename Claim>
__device__ __forceinline__ void nb_seed(const int32_t *__restrict__ roots, const int n_roots, const int n, uint32_t *tail, int32_t *queue, Claim &&claim)
{
    const int lane = threadIdx.x & 63;
    const int stride = int(gridDim.x * blockDim.x);
    const int rounds = (n_roots + stride - 1) / stride;
    for (int r = 0; r < rounds; ++r) {
        const int i = r * stride + int(blockIdx.x * blockDim.x + threadIdx.x);
        bool won = false;
        int node = -1;
        if (i < n_roots) {
            node = roots[i];
            won = uint32_t(node) < uint32_t(n) && claim(node);
        }
        wave_append(won, tail, queue, node, uint32_t(n), lane); // (at most one entry per node: below n)
    }
}

// one launch of a kernel that is a template of <DIR, SCAN>, chosen by the `direction` and `scan` of the launch function, on its
// stream `s`; an unknown direction ends the function
#define RM_NB_BY_DIR_SCAN(kern, grid, block, ...)                                                                             \
    do {                                                                                                                      \
        if (direction == RM_NB_HEARD_BY && scan) RM_KLAUNCH((kern<RM_NB_HEARD_BY, true>), grid, block, 0, s, __VA_ARGS__);    \
        else if (direction == RM_NB_HEARD_BY) RM_KLAUNCH((kern<RM_NB_HEARD_BY, false>), grid, block, 0, s, __VA_ARGS__);      \
        else if (direction == RM_NB_HEARS && scan) RM_KLAUNCH((kern<RM_NB_HEARS, true>), grid, block, 0, s, __VA_ARGS__);     \
        else if (direction == RM_NB_HEARS) RM_KLAUNCH((kern<RM_NB_HEARS, false>), grid, block, 0, s, __VA_ARGS__);            \
        else return hipErrorInvalidValue;                                                                                     \
    } while (0)

// One wave walks the pairs of `node` (wave-uniform, inside the table) in rounds of up to 64, a lane each.
// DIR = RM_NB_HEARD_BY: the node transmits, the pairs' far ends are receivers; RM_NB_HEARS: it receives, the far ends transmit
// with their own table txpower (prep / off_list: what k_nb_prep left).  SCAN: every node of the table is evaluated exactly (no
// box, no fp32 test) -- the path for a table whose boxes say nothing (not sorted, an fp32 frame beyond the plan's slack, no finite
// cut-off).  level: a pair is a link iff its rssi >= level, and the boxes' cut-off is taken there (the sensitivity, or above it).
// want(far): a lane's far end is of interest at all -- asked before the pair's arithmetic, which a `false` skips.
// round(link, rssi, far): called by the whole wave once per round (it may ballot); far ends are distinct inside a round.
template <int DIR, bool SCAN, typename Want, typename Round>
__device__ __forceinline__ void nb_walk(const NodesDev &nd, const ModelDev &m, const unsigned long long *prep, const int32_t *off_list, const int node, const double level,
                  const int lane, Want &&want, Round &&round)
{
    const SrcRecord sj = nd.srec[node];
    // the Tx record rm_tick_run_sources_device builds for the node (make_tx_record): the transmitter of HEARD_BY
    rm_tx_record rec;
    rec.x = sj.x;
    rec.y = sj.y;
    rec.z = sj.z;
    rec.txpower = sj.txpower;
    rec.txprob = sj.txprob;
    rec.start_us = 0;
    rec.air_us = 0;
    rec.src = node;
    rec.channel = sj.channel;
    const int ch = sj.channel;
    // HEARS: the node is the receiver of all its pairs -- its own tests once
    const bool listens = (DIR == RM_NB_HEARD_BY) || (nd.senabled[node] != 0 && !(nd.srxprob[node] <= 0.0));

    // the pair (node, receiver at engine position p), eval_link<RM_MODEL_LOGDIST>'s tests and arithmetic
    auto pair_rx = [&](const int p, bool &link, double &rssi, int &far) {
        const RxRecord rx = nd.rec[p];
        far = rx.orig;
        link = false;
        if (far == node || !rx.enabled || rx.channel != ch || rx.rxprob <= 0.0 || !want(far)) return;
        rssi = logdist_rssi(m, rec, rx.x, rx.y, rx.z, far);
        link = rssi >= level;
    };
    // the pair (transmitter c, node)
    auto pair_tx = [&](const int c, bool &link, double &rssi, int &far) {
        const SrcRecord sc = nd.srec[c];
        far = c;
        link = false;
        if (c == node || sc.channel != ch || !want(c)) return;
        rm_tx_record rc = rec;
        rc.x = sc.x;
        rc.y = sc.y;
        rc.z = sc.z;
        rc.txpower = sc.txpower;
        rc.src = c;
        rssi = logdist_rssi(m, rc, sj.x, sj.y, sj.z, node);
        link = rssi >= level;
    };

    if (listens && SCAN) {
        for (int p0 = 0; p0 < nd.n_rx; p0 += 64) { // wave-uniform
            const int p = p0 + lane;
            bool link = false;
            double rssi = 0.0;
            int far = -1;
            if (p < nd.n_rx) {
                if (DIR == RM_NB_HEARD_BY) pair_rx(p, link, rssi, far);
                else pair_tx(nd.orig[p], link, rssi, far);
            }
            round(link, rssi, far);
        }
    } else if (listens) {
        // the cut-off: the sweep's pre-filter record at the level -- for HEARS with the table's largest txpower, which bounds
        // every far end's reach (the fp32 distance is symmetric)
        rm_tx_record pre = rec;
        if (DIR == RM_NB_HEARS) pre.txpower = nb_key_value(prep[0]);
        float4 f;
        double thr64;
        tx_prefilter_at(m, level, pre, f, thr64);
        if (f.w >= 0.f) {
            const uint32_t chbit = 1u << (uint32_t(ch) & 31u);
            const int n_groups = (nd.n_rx + kGroup - 1) / kGroup;
            const int n_boxes = (n_groups + 15) / 16;
            for (int b0 = 0; b0 < n_boxes; b0 += 64) { // the boxes of 1024 receivers, a lane each
                const int b = b0 + lane;
                const bool near = b < n_boxes && (nd.wg_chmask[b] & chbit) != 0u && box_near(nd.wg_box_xy[b], nd.wg_box_z[b], f);
                uint64_t bm = ballot64(near);
                while (bm) {
                    const int bb = b0 + __ffsll((long long)bm) - 1;
                    bm &= bm - 1ull;
                    const int g = bb * 16 + (lane & 15); // its 16 group boxes
                    const bool gnear = lane < 16 && g < n_groups && (nd.grp_chmask[g] & chbit) != 0u && box_near(nd.bbox_xy[g], nd.bbox_z[g], f);
                    uint64_t gm = ballot64(gnear);
                    while (gm) {
                        const int p = (bb * 16 + __ffsll((long long)gm) - 1) * kGroup + lane; // a near group's 64 receivers
                        gm &= gm - 1ull;
                        bool link = false;
                        double rssi = 0.0;
                        int far = -1;
                        if (p < nd.n_rx) {
                            const float4 v = nd.rxf[p];
                            const float s2 = dist2_f32(v.x - f.x, v.y - f.y, v.z - f.z);
                            if (s2 <= f.w && __float_as_int(v.w) == ch) {
                                if (DIR == RM_NB_HEARD_BY) pair_rx(p, link, rssi, far);
                                else pair_tx(nd.orig[p], link, rssi, far);
                            }
                        }
                        round(link, rssi, far);
                    }
                }
            }
            if (DIR == RM_NB_HEARS) {
                // a radio that is off has no pre-filter record and is in no box, but transmits all the same (the rule takes
                // enabled_s out): those nodes, listed by k_nb_prep, are evaluated one by one
                const unsigned long long off_cnt = prep[1];
                const int n_off = uniform_i(off_cnt < (unsigned long long)nd.n ? int(off_cnt) : nd.n);
                for (int i0 = 0; i0 < n_off; i0 += 64) {
                    const int i = i0 + lane;
                    bool link = false;
                    double rssi = 0.0;
                    int far = -1;
                    if (i < n_off) pair_tx(off_list[i], link, rssi, far);
                    round(link, rssi, far);
                }
            }
        }
    }
}

} // namespace rm
