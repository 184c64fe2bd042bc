// rm_rankframes.hip -- a rank's frame lists of a batch of gathered ticks, the check of frames kept on the air against the partition's box
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
#include "rm_device.hpp"

namespace rm {

// The union of the first n_wg filter-workgroup boxes and channel masks, by a workgroup of exactly kBlock threads (strided over
// the boxes, over the lanes, through LDS across the waves): every thread gets the union.  One call per kernel: the LDS words are
// the function's own.
RM_D BoxUnion wg_boxes_union(const NodesDev &nd, const int n_wg)
{
    __shared__ BoxUnion s_u[kWavesPerBlock];
    BoxUnion u = box_union_empty();
    for (int w = int(threadIdx.x); w < n_wg; w += kBlock) box_union_add(u, nd.wg_box_xy[w], nd.wg_box_z[w], nd.wg_chmask[w]);
    box_union_lanes(u, 32);
    if ((threadIdx.x & 63) == 0) s_u[wave_index()] = u;
    __syncthreads();
    for (int w = 0; w < kWavesPerBlock; ++w) box_union_add(u, s_u[w].xy, s_u[w].z, s_u[w].chmask);
    return u;
}

// A rank's frame list (one workgroup per tick of a batch of GATHERED ticks over a receiver partition).  The all-gather hands
// every rank the source indices of all ranks' frames; a region of the plane hears nothing of most of them, and what every
// later stage did per frame -- the pre-pass, the near-frame lists, the per-frame scans, the reorder stage's walk, the
// interference stages' index -- it did for all of them: a rank's time did not follow its links.  Here the tick's frames are
// tested ONCE against the union of the partition's filter-workgroup boxes with the workgroups' own expression (so a frame
// that could pass any workgroup's test passes this one: monotone in every |d|, the union box contains every box) and the
// survivors are compacted IN ORDER: the tick goes on as a tick of those frames only, its descriptor patched here on the
// device (n_active, n_cnt) -- the host sizes grids for all frames and never learns the count.  This launch is also the
// listed frames' pre-pass (k_tick_prep_batch is not launched for such a batch): their on-air records, their pre-filter
// records at the SWEEP's candidate level (sweep_level: a batch of overlapping SINR ticks sweeps at the sensitivity and lists
// at the interference floor), the counters later kernels add to.  Packets keep their global numbers: fl_map (local ->
// gathered slot) for the records' packet column, fl_lb (gathered slot -> listed frames before it) for the offsets by global
// number, and the per-packet Tx-failure flag of EVERY gathered slot is written here (it depends on the source's
// txProbability alone).  A frame whose source is one of the partition's own receivers is always kept (half duplex asks for
// no reach).  The ranks' node-table digests ride in the gathered blocks: a rank that built its records from another table
// than this one flags every tick (RM_ERR_STATE).
// (256 threads per tick, eight frames per thread and round -- 2048 frames per round, their loads all issued before any is used:
// a tick of a thousand frames is one round of independent round trips.  A workgroup of 1024 threads per tick was measured: alone
// on the device 36 us per 512 ticks, but 243 us with two other contexts' kernels in flight -- it waits for a compute unit with
// room for all sixteen of its waves.)
constexpr int kRfThreads = kBlock; // (wg_boxes_union's workgroup, as k_cull_check's 256)
constexpr int kRfPer = 8;

// a window of frames selected for this partition (CullEntry) that is still on the air at t_begin: have the partition's receivers left its box?
RM_D bool cull_moved(const CullEntry &e, const int64_t t_begin, const BoxUnion &p)
{
    return e.end_us > t_begin && (p.xy.x < e.lo[0] || p.xy.y < e.lo[1] || p.z.x < e.lo[2] || p.xy.z > e.hi[0] || p.xy.w > e.hi[1] || p.z.y > e.hi[2]);
}
__global__ void __launch_bounds__(kRfThreads) k_rank_frames(const NodesDev nd, const ModelDev m, TickDev *__restrict__ ticks, const RankFramesArgs a)
{
    constexpr int kWaves = kRfThreads / 64;
    __shared__ uint32_t s_wcnt[kRfPer][kWaves];
    TickDev &t = ticks[blockIdx.x];
    const int tid = int(threadIdx.x), lane = tid & 63, wave = wave_index();
    const int T = t.n_pub;
    if (a.digest_off >= 0)
        for (int r = tid; r < a.world; r += kRfThreads) {
            const int32_t *d = a.gather_base + size_t(r) * size_t(a.gather_block) + size_t(a.digest_off);
            const uint64_t v = uint64_t(uint32_t(d[0])) | (uint64_t(uint32_t(d[1])) << 32);
            if (v != a.mine) t.stage_count[6] = 3u; // read as RM_ERR_STATE with the tick's result
        }
    if (T <= 0 || t.gather_idx == nullptr) return; // block-uniform: no list for this tick (the digests were all there was to do)
    // ---- the first round's source indices: requested before anything else
    int src[kRfPer];
    auto request = [&](const int i0) {
#pragma unroll
        for (int u = 0; u < kRfPer; ++u) {
            const int i = i0 + u * kRfThreads + tid;
            src[u] = -1;
            if (i < T) src[u] = t.gather_idx[size_t(i / t.gather_slots) * size_t(t.gather_stride) + size_t(i % t.gather_slots)];
        }
    };
    request(0);
    tick_zero_duties(t, tid, kRfThreads); // ---- k_tick_prep's duties for the counters
    // ---- the partition's box: the union of its filter workgroups' boxes and channel masks
    BoxUnion part = wg_boxes_union(nd, (t.n_rx + kGroup * 16 - 1) / (kGroup * 16));
    if (a.ring != nullptr) { // (block-uniform) frames that stay on the air: is every receiver still where the frames on the air were selected for?
        if (tid < kCullRing && tid != a.ring_slot && cull_moved(a.ring[tid], a.t_first, part)) t.stage_count[6] = 4u; // read as RM_ERR_STATE with the tick's result
        if (blockIdx.x == 0 && tid == 0) {
            CullEntry e;
            e.lo[0] = part.xy.x - a.margin, e.lo[1] = part.xy.y - a.margin, e.lo[2] = part.z.x - a.margin;
            e.hi[0] = part.xy.z + a.margin, e.hi[1] = part.xy.w + a.margin, e.hi[2] = part.z.y + a.margin;
            e.end_us = a.batch_end;
            a.ring[a.ring_slot] = e;
        }
    }
    part.xy.x -= a.margin, part.xy.y -= a.margin, part.z.x -= a.margin, part.xy.z += a.margin, part.xy.w += a.margin, part.z.y += a.margin;
    if (!a.use_chmask) part.chmask = 0xFFFFFFFFu;
    const bool draws_possible = (m.kind == RM_MODEL_UDGM || m.kind == RM_MODEL_N2N || m.kind == RM_MODEL_LOGDIST);
    uint32_t base = 0; // frames listed so far (block-uniform)
    for (int i0 = 0; i0 < T; i0 += kRfPer * kRfThreads) { // block-uniform: one round per 2048 frames
        if (i0) request(i0);
        // ---- which frames matter here
        uint64_t hms[kRfPer];
        float4 fl[kRfPer]; // pre-filter records at the LIST's level
#pragma unroll
        for (int u = 0; u < kRfPer; ++u) {
            const int i = i0 + u * kRfThreads + tid;
            bool hit = false;
            fl[u] = make_float4(0.f, 0.f, 0.f, -1.f);
            if (i < T) {
                const rm_tx_record r = make_tx_record(nd, src[u], t.src_start_us, t.src_air_us);
                t.pkt_interference[i] = (draws_possible && tx_success(m, r) <= 0.0) ? 1 : 0; // (write_pkt_interference's rule, by global number)
                if (r.src >= 0) {
                    double thr64;
                    tx_prefilter(m, r, fl[u], thr64);
                    hit = box_near(part.xy, part.z, fl[u]) && ((part.chmask >> (uint32_t(r.channel) & 31u)) & 1u) != 0u;
                    if (!hit) hit = engine_pos(nd, r.src) >= 0; // a receiver of this partition that is on the air itself: half duplex
                }
            }
            hms[u] = ballot64(hit);
            if (lane == 0) s_wcnt[u][wave] = uint32_t(__popcll(hms[u]));
        }
        __syncthreads();
        // ---- ordered compaction: frame i = i0 + u * 256 + tid comes after the frames of the chunks before u and of the waves before its own
#pragma unroll
        for (int u = 0; u < kRfPer; ++u) {
            const int i = i0 + u * kRfThreads + tid;
            uint32_t k = base + lane_prefix(hms[u]);
            uint32_t tot = 0;
            for (int w = 0; w < kWaves; ++w) {
                const uint32_t c = s_wcnt[u][w];
                if (w < wave) k += c;
                tot += c;
            }
            base += tot;
            if (i < T) t.fl_lb[i] = k;
            if (i < T && ((hms[u] >> lane) & 1ull)) {
                // (the listed frames' records are fetched again -- a fifth of the frames, L2-resident -- rather than kept for all eight)
                const rm_tx_record r = make_tx_record(nd, src[u], t.src_start_us, t.src_air_us);
                t.fl_map[k] = i;
                t.tx_build[k] = r;
                float4 f = fl[u];
                if (a.sweep_level != m.ld_level) { // (the sweep's own cut-off: the medium without SINR sweeps at the sensitivity)
                    double thr64;
                    tx_prefilter_at(m, a.sweep_level, r, f, thr64);
                }
                t.p_txf[k] = f;
                t.p_ch[k] = r.channel;
                t.p_src[k] = r.src;
                t.p_inv[k] = prefilter_inv(m, f);
            }
        }
        __syncthreads(); // (the next round's counts overwrite s_wcnt)
    }
    // (records kept on the air: the slots behind the listed frames hold padding, as the unlisted frames' own slots would
    // have -- whoever walks the window later finds records everywhere)
    if (t.fl_pad)
        for (int e = int(base) + tid; e < T; e += kRfThreads) t.tx_build[e] = make_tx_record(nd, -1, t.src_start_us, 0);
    if (tid == 0) {
        t.fl_lb[T] = base;
        t.n_active = int(base);
        t.n_cnt = max(kTxChunk, int((base + uint32_t(kTxChunk) - 1u) / uint32_t(kTxChunk)) * kTxChunk);
        t.gather_idx = nullptr; // (the records are in place: nothing of the gathered layout is needed any more)
        if (t.fl_ov_n_new) *t.fl_ov_n_new = int(base);
    }
}

// a lone tick over a window of frames that were selected for this partition (CullEntry): the same comparison, on its own
__global__ void __launch_bounds__(kBlock) k_cull_check(const NodesDev nd, const CullEntry *__restrict__ ring, int64_t t_begin, uint32_t *flag_word)
{
    const BoxUnion part = wg_boxes_union(nd, (nd.n_rx + kGroup * 16 - 1) / (kGroup * 16));
    if (threadIdx.x < kCullRing && cull_moved(ring[threadIdx.x], t_begin, part)) *flag_word = 4u;
}

hipError_t launch_cull_check(hipStream_t s, const NodesDev &nd, const CullEntry *ring, int64_t t_begin, uint32_t *flag_word)
{
    RM_KLAUNCH(k_cull_check, dim3(1), dim3(kBlock), 0, s, nd, ring, t_begin, flag_word);
    return hipGetLastError();
}

hipError_t launch_rank_frames(hipStream_t s, const NodesDev &nd, const ModelDev &m, TickDev *dev_ticks, int n, const RankFramesArgs &a)
{
    if (n <= 0) return hipSuccess;
    RM_KLAUNCH(k_rank_frames, dim3(n), dim3(kRfThreads), 0, s, nd, m, dev_ticks, a);
    return hipGetLastError();
}

} // namespace rm
