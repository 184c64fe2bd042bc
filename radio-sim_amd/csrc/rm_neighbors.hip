// rm_neighbors.hip -- the neighbour query: each node's K strongest potential links; the
// device-side validation of rm_linkstats_watch_device
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// Not the source-candidate cache (rm_nbrcache.hip): this is a read-only query over the node table and the model.
#include "rm_nbwalk.hpp" // (nb_value_key, nb_key_value, nb_precedes: shared with the hop query)

namespace rm {

// A wave's running top-K, entry i in lane i (K <= 16 <= 64): sorted by the rule, `cnt` entries (wave-uniform).  No LDS and no
// atomics: an insertion is one ballot (how many entries precede the new one) and one shuffle (the rest moves up a lane).
struct NbTop {
    double rssi;
    int node;
    int cnt;
    double kth_rssi; // the last entry of a full list (wave-uniform)
    int kth_node;
};

RM_D void nb_insert(NbTop &t, const int K, const int lane, const double r, const int n)
{
    const bool first = lane < t.cnt && nb_precedes(t.rssi, t.node, r, n);
    const int pos = __popcll(ballot64(first)); // (the list is sorted: the entries that precede the new one are lanes 0 .. pos - 1)
    const double ur = __shfl_up(t.rssi, 1);
    const int un = __shfl_up(t.node, 1);
    if (lane == pos) {
        t.rssi = r;
        t.node = n;
    } else if (lane > pos && lane <= t.cnt) {
        t.rssi = ur;
        t.node = un;
    }
    t.cnt = min(t.cnt + 1, K);
    if (t.cnt == K) {
        t.kth_rssi = __shfl(t.rssi, K - 1);
        t.kth_node = __shfl(t.node, K - 1);
    }
}

// one round of up to 64 evaluated pairs (a lane each): the links are counted, and those that beat the current K-th are inserted
// best first -- a wave-wide maximum by the rule's comparison per insertion, until no lane contends any more
RM_D void nb_absorb(NbTop &t, int &degree, const int K, const int lane, const bool link, const double rssi, const int far)
{
    const uint64_t lm = ballot64(link);
    if (!lm) return;
    degree += __popcll(lm);
    bool open = link;
    for (;;) {
        const bool beats = open && (t.cnt < K || nb_precedes(rssi, far, t.kth_rssi, t.kth_node));
        if (!ballot64(beats)) break;
        double br = rssi;
        int bn = far;
        bool bv = beats;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double o_r = __shfl_xor(br, d);
            const int o_n = __shfl_xor(bn, d);
            const bool o_v = __shfl_xor(int(bv), d) != 0;
            if (o_v && (!bv || nb_precedes(o_r, o_n, br, bn))) {
                br = o_r;
                bn = o_n;
                bv = true;
            }
        }
        if (beats && far == bn) open = false; // (far ends are distinct inside a round)
        nb_insert(t, K, lane, br, bn);
    }
}

// DIR = RM_NB_HEARD_BY: the queried node transmits, the pairs' far ends are receivers; RM_NB_HEARS: it receives, the far ends
// transmit with their own table txpower.  SCAN: every node of the table is evaluated exactly (no box, no fp32 test) -- the path
// for a table whose boxes say nothing (not sorted, an fp32 frame beyond the plan's slack, no finite cut-off).
template <int DIR, bool SCAN>
__global__ void __launch_bounds__(kBlock) k_nb_query(const NodesDev nd, const ModelDev m, const NbDev q)
{
    const int lane = threadIdx.x & 63;
    const int e = int(blockIdx.x) * kNbWaves + wave_index();
    if (e >= q.n) return;
    // all nodes: in the receiver table's engine order, so that a workgroup's waves walk the same boxes
    const int node = uniform_i(q.list ? q.list[e] : nd.orig[e]);
    const size_t row = size_t(q.list ? e : node);
    const int K = q.K;
    NbTop top;
    top.rssi = 0.0;
    top.node = -1;
    top.cnt = 0;
    top.kth_rssi = 0.0;
    top.kth_node = -1;
    int degree = 0;
    if (uint32_t(node) < uint32_t(nd.n)) {
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
            if (far == node || !rx.enabled || rx.channel != ch || rx.rxprob <= 0.0) return;
            rssi = logdist_rssi(m, rec, rx.x, rx.y, rx.z, far);
            link = rssi >= m.ld_sens;
        };
        // the pair (transmitter c, node)
        auto pair_tx = [&](const int c, bool &link, double &rssi, int &far) {
            const SrcRecord sc = nd.srec[c];
            far = c;
            link = false;
            if (c == node || sc.channel != ch) return;
            rm_tx_record rc = rec;
            rc.x = sc.x;
            rc.y = sc.y;
            rc.z = sc.z;
            rc.txpower = sc.txpower;
            rc.src = c;
            rssi = logdist_rssi(m, rc, sj.x, sj.y, sj.z, node);
            link = rssi >= m.ld_sens;
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
                nb_absorb(top, degree, K, lane, link, rssi, far);
            }
        } else if (listens) {
            // the cut-off: the sweep's pre-filter record at the sensitivity -- for HEARS with the table's largest txpower, which bounds
            // every far end's reach (the fp32 distance is symmetric)
            rm_tx_record pre = rec;
            if (DIR == RM_NB_HEARS) pre.txpower = nb_key_value(q.prep[0]);
            float4 f;
            double thr64;
            tx_prefilter_at(m, m.ld_sens, pre, f, thr64);
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
                            nb_absorb(top, degree, K, lane, link, rssi, far);
                        }
                    }
                }
                if (DIR == RM_NB_HEARS) {
                    // a radio that is off has no pre-filter record and is in no box, but transmits all the same (the rule takes
                    // enabled_s out): those nodes, listed by k_nb_prep, are evaluated one by one
                    const unsigned long long off_cnt = q.prep[1];
                    const int n_off = uniform_i(off_cnt < (unsigned long long)nd.n ? int(off_cnt) : nd.n);
                    for (int i0 = 0; i0 < n_off; i0 += 64) {
                        const int i = i0 + lane;
                        bool link = false;
                        double rssi = 0.0;
                        int far = -1;
                        if (i < n_off) pair_tx(q.off_list[i], link, rssi, far);
                        nb_absorb(top, degree, K, lane, link, rssi, far);
                    }
                }
            }
        }
    }
    if (lane < K) {
        const bool have = lane < top.cnt;
        q.peer[row * size_t(K) + lane] = have ? top.node : -1;
        if (q.rssi) q.rssi[row * size_t(K) + lane] = have ? f2u(top.rssi) : kNbNoRssi;
    }
    if (lane == 0 && q.degree) q.degree[row] = degree;
}

// What a HEARS query needs of the whole table, per call (the table may have been patched since the last one): prep[0] the largest
// txpower as an ordered key (0: no node has one that is a number), prep[1] the number of nodes whose radio is off, off_list those
// nodes in any order.  prep is zeroed in front of the launch.
__global__ void __launch_bounds__(kBlock) k_nb_prep(const NodesDev nd, unsigned long long *prep, int32_t *off_list)
{
    const int lane = threadIdx.x & 63;
    unsigned long long key = 0ull;
    const int stride = int(gridDim.x * blockDim.x);
    const int rounds = (nd.n + stride - 1) / stride;
    for (int r = 0; r < rounds; ++r) { // workgroup-uniform: whole waves reach the ballot
        const int i = r * stride + int(blockIdx.x * blockDim.x + threadIdx.x);
        bool off = false;
        if (i < nd.n) {
            key = max(key, nb_value_key(nd.stxpower[i]));
            off = nd.senabled[i] == 0;
        }
        const uint64_t om = ballot64(off);
        if (om) {
            unsigned long long base = 0ull;
            if (lane == 0) base = atomicAdd(&prep[1], (unsigned long long)__popcll(om));
            base = (unsigned long long)__shfl((long long)base, 0);
            if (off) off_list[base + lane_prefix(om)] = i;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, d));
    if (lane == 0 && key != 0ull) atomicMax(&prep[0], key);
}

// rm_linkstats_validate's rules for rows in device memory, a row per thread: the node in range and listed once (mark: a word per
// node, `stamp` is this call's), every entry -1 or a node index other than the row's own, the entries distinct.  A row that breaks
// one raises *bad.
__global__ void __launch_bounds__(kBlock) k_nb_watch_check(const int32_t *__restrict__ nodes, int n, const int32_t *__restrict__ peers, int n_nodes, int K,
                                                          uint32_t *mark, uint32_t stamp, uint32_t *bad)
{
    const int r = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n) return;
    const int node = nodes ? nodes[r] : r;
    bool ok = node >= 0 && node < n_nodes;
    if (ok && nodes) ok = atomicExch(&mark[node], stamp) != stamp;
    const int32_t *row = peers + size_t(r) * size_t(K);
    for (int k = 0; ok && k < K; ++k) {
        const int32_t p = row[k];
        if (p == -1) continue;
        ok = p >= 0 && p < n_nodes && p != node;
        for (int j = 0; ok && j < k; ++j) ok = row[j] != p;
    }
    if (!ok) *bad = 1u;
}

hipError_t launch_nb_prep(hipStream_t s, const NodesDev &nd, unsigned long long *prep, int32_t *off_list)
{
    // (a few workgroups: the pass reads 9 bytes a node and ends in two atomics per wave)
    RM_KLAUNCH(k_nb_prep, dim3(max(1, min(cdiv(nd.n, kBlock), 64))), dim3(kBlock), 0, s, nd, prep, off_list);
    return hipGetLastError();
}

hipError_t launch_nb_query(hipStream_t s, const NodesDev &nd, const ModelDev &m, const NbDev &q, int direction, bool scan)
{
    if (q.n < 1) return hipSuccess;
    if (q.K < 1 || q.K > RM_NB_MAX_K || !q.peer) return hipErrorInvalidValue;
    const dim3 grid(cdiv(q.n, kNbWaves)), block(kBlock);
    if (direction == RM_NB_HEARS) {
        const hipError_t e = launch_nb_prep(s, nd, q.prep, q.off_list);
        if (e != hipSuccess) return e;
    }
    RM_NB_BY_DIR_SCAN(k_nb_query, grid, block, nd, m, q);
    return hipGetLastError();
}

hipError_t launch_nb_watch_check(hipStream_t s, const int32_t *nodes, int n, const int32_t *peers, int n_nodes, int K, uint32_t *mark, uint32_t stamp,
                                 uint32_t *bad)
{
    if (n < 1) return hipSuccess;
    RM_KLAUNCH(k_nb_watch_check, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, nodes, n, peers, n_nodes, K, mark, stamp, bad);
    return hipGetLastError();
}

} // namespace rm
