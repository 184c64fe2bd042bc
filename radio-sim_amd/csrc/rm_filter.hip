// rm_filter.hip -- the all-pairs sweep: its grid and two-level (per tick, sixteen ticks) forms, the pre-pass, the near-frame lists, the planner
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
#include "rm_device.hpp"

#include <stdlib.h>
#include <string.h>

namespace rm {

// ============================================================================ shared pieces of the sweeps
// A wave's receivers: one per lane in each of its RPT groups, resident in registers for all it sweeps, with the groups' boxes
// and channel masks and (two-level forms) the union of the workgroup's 4 * RPT groups.  F64: the fp64 positions as well.
template <int RPT, bool F64 = false> struct WgRx {
    float fx[RPT], fy[RPT], fz[RPT];
    int fch[RPT], forig[RPT];
    double gx[F64 ? RPT : 1], gy[F64 ? RPT : 1], gz[F64 ? RPT : 1];
    float4 bxy[RPT];
    float2 bz[RPT];
    uint32_t bmask[RPT]; // the groups' channel masks
    BoxUnion w;          // ... and the workgroup's box and mask
};

// Where the records of the (up to) 64 frames a wave sweeps at a time are staged in LDS: frame ti's record is at [c0 + ti].
struct Staged {
    const float4 *txf;   // pre-filter record
    const int *ch;       // channel
    const float *inv;    // (SHADOW) bins / thr of the frame (0: table not usable for it)
    const int *src;      // (SHADOW) source node
    const uint32_t *tbl; // (SHADOW) the link-hash table
    const double *td;    // (F64) [(c0 + ti) * 4]: position and threshold in fp64
    int c0;
};

// Where a wave's candidates go: one run per wave in one shard of one tick: one atomic reserves the contiguous run of
// candidate entries, the frames' blocks follow each other inside it in frame order.  Frame ti's packet is e0 + ti.
struct RunPerWave {
    const TickDev &t;
    uint32_t shard;
    int e0;
    RM_D int pkt(const int ti) const { return e0 + ti; }
    RM_D const TickDev &tick(const int) const { return t; }
    // my_total: the candidates of the frame in this lane; returns the lanes whose frames have room (my_base: where)
    RM_D uint64_t reserve(const uint32_t my_total, const int lane, uint32_t &my_base) const
    {
        const int my_e = pkt(lane);
        // candidate links per frame (frames that get verdicts only): sizes the frame's segment
        if (!t.use_matrix && my_total != 0u && t.first_eval + my_e >= t.first_new) atomicAdd(&t.cand_tot[my_e - t.cnt_base], my_total);
        const uint32_t inc = wave_inclusive_scan(my_total, lane);
        const uint32_t wave_total = __shfl(inc, 63);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&t.shard_count[shard * kShardStride], wave_total);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base + wave_total > t.seg_cap) { // the shard is full: drop the run, flag the tick
            if (lane == 0) t.stage_count[1] = 1u;
            return 0;
        }
        my_base = shard * t.seg_cap + base + inc - my_total;
        return ballot64(my_total != 0u);
    }
};
// which staged frames (one per lane, nt of them) can reach which of the wave's receiver groups: the frame against the group's
// bounding box and channel mask, one ballot per group; returns the frames near any
template <int RPT, bool F64>
RM_D uint64_t near_groups(const WgRx<RPT, F64> &rx, const Staged &s, const int nt, const int slab, const int n_rx, const int lane, uint64_t (&near)[RPT])
{
    const float4 tf = s.txf[s.c0 + min(lane, nt - 1)];
    const uint32_t tchb = uint32_t(s.ch[s.c0 + min(lane, nt - 1)]) & 31u;
    uint64_t todo = 0;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        near[r] = 0;
        if ((slab * RPT + r) * kGroup < n_rx) near[r] = ballot64(lane < nt && box_near(rx.bxy[r], rx.bz[r], tf) && ((rx.bmask[r] >> tchb) & 1u) != 0u);
        todo |= near[r];
    }
    return todo;
}

// The filter of one wave over its RPT receiver groups (jbase: the first receiver) and the staged frames `todo` (near[r]: those
// of group r).  s_mask: the wave's own [kTxChunk][RPT] words of LDS.
// (The grid form's pass 1, reservation and pass 2.  The two-level forms keep these steps as their own text: through this function
// k_filter_wg<4|2, true> lose an occupancy step to scalar-register spills and k_filter_wg_group measures 1.5 % slower.  It stays a
// function with its reservation as RunPerWave: written into k_filter's body, k_filter<1, false, true, true> needs 106 scalar
// registers and loses a step as well.)
template <int RPT, bool SHADOW, bool F64>
RM_D void sweep_two_pass(const ModelDev &m, const Staged &s, const WgRx<RPT, F64> &rx, const uint64_t (&near)[RPT], const uint64_t todo,
                         uint64_t (*s_mask)[RPT], const RunPerWave &res, const int jbase, const int lane)
{
    // pass 1: per near frame, the candidate ballots of the RPT groups; lane ti keeps frame ti's count
    uint32_t my_total = 0;
    uint64_t walk = todo;
    while (walk) {
        const int ti = __ffsll((long long)walk) - 1; // wave-uniform
        walk &= walk - 1;
        const float4 tf = s.txf[s.c0 + ti];
        const int tch = s.ch[s.c0 + ti];
        uint64_t mask[RPT];
        uint32_t total = 0;
        if (F64) {
            const double *td = s.td + (s.c0 + ti) * 4;
            const double px = td[0], py = td[1], pz = td[2], thr = td[3];
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const double dx = px - rx.gx[r], dy = py - rx.gy[r], dz = pz - rx.gz[r];
                const double s2 = dx * dx + dy * dy + dz * dz;
                mask[r] = ballot64((s2 <= thr) && (rx.fch[r] == tch));
                total += uint32_t(__popcll(mask[r]));
            }
        } else {
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                mask[r] = 0;
                if ((near[r] >> ti) & 1ull) { // wave-uniform
                    const float s2 = dist2_f32(rx.fx[r] - tf.x, rx.fy[r] - tf.y, rx.fz[r] - tf.z);
                    bool hit = (s2 <= tf.w) && (rx.fch[r] == tch);
                    if (SHADOW && hit) hit = shadow_pass(m, s.tbl, s2, s.inv[s.c0 + ti], s.src[s.c0 + ti], rx.forig[r]);
                    mask[r] = ballot64(hit);
                    total += uint32_t(__popcll(mask[r]));
                }
            }
        }
        if (total) {
            if (lane == ti) my_total = total;
            if (lane < RPT) {
                uint64_t v = mask[0];
#pragma unroll
                for (int r = 1; r < RPT; ++r) v = (lane == r) ? mask[r] : v;
                s_mask[ti][lane] = v;
            }
        }
    }
    if (ballot64(my_total != 0u) == 0) return; // the common case: far from every staged frame

    uint32_t my_base = 0;
    walk = res.reserve(my_total, lane, my_base);

    // pass 2: fill the blocks in receiver order
    while (walk) {
        const int ti = __ffsll((long long)walk) - 1;
        walk &= walk - 1;
        const uint32_t fbase = uniform_u(uint32_t(__shfl(int(my_base), ti)));
        const int e_ti = res.pkt(ti);
        const TickDev &T = res.tick(ti);
        uint32_t pre = 0;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const uint64_t mk = s_mask[ti][r];
            if (mk == 0) continue;
            if ((mk >> lane) & 1ull) {
                const uint32_t idx = fbase + pre + lane_prefix(mk);
                T.st_pkt[idx] = e_ti;
                T.st_dst[idx] = jbase + r * kGroup + lane;
                if (T.use_matrix) T.st_blk[idx] = fbase; // the run's base: only the ordered scatter of unsorted tables ranks inside it
            }
            pre += uint32_t(__popcll(mk));
        }
    }
}

// ============================================================================ the grid filter
// k_filter: one workgroup per (4 waves x RPT receiver groups, tile of 64 frames) -- the general variant (fp64 frame, unsorted
// tables): the tile's pre-filter records are computed on the fly from the on-air records.
template <int RPT, bool F64, bool BBOX, bool SHADOW>
__global__ void __launch_bounds__(kBlock, F64 ? 2 : 6) k_filter(const NodesDev nd, const ModelDev m, const TickDev t)
{
    __shared__ float4 s_txf[kTxChunk];
    __shared__ int s_ch[kTxChunk];
    __shared__ double s_td[F64 ? kTxChunk * 4 : 1];
    __shared__ uint64_t s_mask[kWavesPerBlock][kTxChunk][RPT]; // candidate ballots of the near frames
    __shared__ uint32_t s_tbl[SHADOW ? kShadowBins : 1];
    __shared__ float s_inv[SHADOW ? kTxChunk : 1]; // bins / thr of the frame (0: table not usable for it)
    __shared__ int s_src[SHADOW ? kTxChunk : 1];

    const int lane = threadIdx.x & 63;
    const int wave = wave_index();
    const int slab = blockIdx.x * kWavesPerBlock + wave;
    const int chunk = blockIdx.y;
    const int n_eval = t.n_active - t.first_eval;
    const int e0 = chunk * kTxChunk; // eval-relative index of the tile's first frame
    const int nt = min(kTxChunk, n_eval - e0);
    const int jbase = slab * (kGroup * RPT);

    // receivers of this lane (coalesced 16-byte loads), resident in registers for the whole tile;
    // issued before the tile is staged so that both round trips overlap
    WgRx<RPT, F64> rx;
    if (SHADOW) s_tbl[threadIdx.x] = m.shadow_tbl[threadIdx.x]; // kBlock == kShadowBins
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int j = jbase + r * kGroup + lane;
        rx.fx[r] = rx.fy[r] = rx.fz[r] = __builtin_nanf("");
        rx.fch[r] = 0;
        rx.forig[r] = 0;
        if (F64) rx.gx[r] = rx.gy[r] = rx.gz[r] = u2f(0x7FF8000000000000ull);
        if (j < t.n_rx) {
            const float4 v = nd.rxf[j];
            rx.fx[r] = v.x;
            rx.fy[r] = v.y;
            rx.fz[r] = v.z;
            rx.fch[r] = __float_as_int(v.w);
            if (SHADOW) rx.forig[r] = nd.orig[j];
            if (F64 && v.x == v.x) {
                rx.gx[r] = nd.x[j];
                rx.gy[r] = nd.y[j];
                rx.gz[r] = nd.z[j];
            }
        }
        if (BBOX) {
            const int g = slab * RPT + r;
            const bool ok = g * kGroup < t.n_rx;
            rx.bxy[r] = ok ? nd.bbox_xy[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            rx.bz[r] = ok ? nd.bbox_z[g] : make_float2(0.f, 0.f);
            rx.bmask[r] = 0xFFFFFFFFu; // (the grid form tests the channel per receiver only)
        }
    }

    // stage the transmitter tile in LDS: one frame per lane of wave 0, pre-filter record computed
    // on the fly from the on-air record
    if (threadIdx.x < kTxChunk) {
        float4 f = make_float4(0.f, 0.f, 0.f, -1.f);
        double thr64 = -1.0;
        int ch = 0;
        int src_id = -1;
        double px = 0, py = 0, pz = 0;
        if (int(threadIdx.x) < nt) {
            rm_tx_record tx;
            const int abs_i = t.first_eval + e0 + int(threadIdx.x);
            if (t.src_list && abs_i >= t.first_new) { // build mode: a new frame's record comes from the source table
                tx = make_tx_record(nd, t.src_list[abs_i - t.first_new], t.src_start_us, t.src_air_us);
                if (blockIdx.x == 0) t.tx_build[abs_i] = tx;
            } else { // a frame already on the air (or records given by the caller)
                tx = t.tx[abs_i];
                if (t.check_txprob && blockIdx.x == 0 && tx.src >= 0 && tx.txprob > 0.0 && tx.txprob < 1.0) t.stage_count[6] = 2u;
            }
            tx_prefilter(m, tx, f, thr64);
            ch = tx.channel;
            src_id = tx.src;
            px = tx.x;
            py = tx.y;
            pz = tx.z;
        }
        s_txf[threadIdx.x] = f;
        s_ch[threadIdx.x] = ch;
        if (SHADOW) {
            s_inv[threadIdx.x] = prefilter_inv(m, f);
            s_src[threadIdx.x] = src_id;
        }
        if (F64) {
            s_td[threadIdx.x * 4 + 0] = px;
            s_td[threadIdx.x * 4 + 1] = py;
            s_td[threadIdx.x * 4 + 2] = pz;
            s_td[threadIdx.x * 4 + 3] = thr64;
        }
    }
    __syncthreads();
    // the pre-pass's zeroing duties, shared by the x = 0 workgroups.  Every thread of them takes part, also the waves
    // without a slab (a table of fewer than four slabs): they leave only afterwards.
    // (its reset_heads / acc_lo branches never run here: only batches set those, and batches take the two-level form)
    if (blockIdx.x == 0) tick_zero_duties(t, blockIdx.y * kBlock + threadIdx.x, gridDim.y * kBlock);
    if (slab >= t.n_slabs) return;
    if (t.use_matrix) {
        if (e0 >= t.cnt_base) t.cnt[(size_t((e0 - t.cnt_base) / kTxChunk) * t.n_slabs + slab) * 64 + lane] = 0u;
    }

    // which frames of the tile can reach which receiver group (padding frames reach nobody: thr < 0)
    const Staged s{s_txf, s_ch, s_inv, s_src, s_tbl, s_td, 0};
    uint64_t near[RPT];
    uint64_t todo;
    if (BBOX) {
        todo = near_groups(rx, s, kTxChunk, slab, t.n_rx, lane, near);
    } else {
        todo = (nt >= 64) ? ~0ull : ((1ull << nt) - 1ull);
#pragma unroll
        for (int r = 0; r < RPT; ++r) near[r] = todo;
    }
    const RunPerWave res{t, (blockIdx.x + blockIdx.y * gridDim.x) & t.shard_mask, e0};
    sweep_two_pass<RPT, SHADOW, F64>(m, s, rx, near, todo, s_mask[wave], res, jbase, lane);
}

// ============================================================================ two-level filter
// k_tick_prep: one thread per swept frame -- builds the frame's on-air record (build mode) and its
// pre-filter record once per tick, and zeroes the counters later kernels add to.
// k_filter_wg: one workgroup per 4*RPT receiver groups.  Phase A: every thread tests frames
// against the union box of the workgroup's receivers and the near ones are compacted into LDS
// (a few dozen of a thousand at the bench densities).  Phase B: each wave runs the two-pass
// filter of k_filter over chunks of 64 near frames for its own RPT groups.

RM_D void tick_prep_body(const NodesDev &nd, const ModelDev &m, const TickDev &t)
{
    const int n_eval = t.n_active - t.first_eval;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    tick_zero_duties(t, e, gridDim.x * blockDim.x);
    if (t.air.pool != nullptr) { // block-uniform.  SINR with the lists that live across ticks:
        if (blockIdx.x == 0 && threadIdx.x == 0 && t.air.bad[0]) t.stage_count[1] = 1u; // the lists are broken until the host rebuilds them
        // half duplex: every swept frame leaves a SELF entry in its source's list (whole waves allocate together)
        bool want = false;
        int pos = 0;
        rm_tx_record txs{};
        if (e < n_eval) {
            const int ai = t.first_eval + e;
            txs = (t.src_list && ai >= t.first_new) ? make_tx_record(nd, t.src_list[ai - t.first_new], t.src_start_us, t.src_air_us) : t.tx[ai];
            pos = engine_pos(nd, txs.src);
            want = pos >= 0;
        }
        const int aidx = air_alloc(t, want, air_sub(t));
        if (want) air_link(t, aidx, pos, txs.start_us, txs.air_us, 0.0, kAirSelf);
    }
    if (e >= n_eval) return;
    const int abs_i = t.first_eval + e;
    rm_tx_record tx;
    if (t.src_list && abs_i >= t.first_new) {
        tx = make_tx_record(nd, t.src_list[abs_i - t.first_new], t.src_start_us, t.src_air_us);
        t.tx_build[abs_i] = tx;
    } else if (t.gather_idx) { // (batches only: first_eval == first_new == 0) the gathered source indices: the record is built here
        tx = make_tx_record(nd, t.gather_idx[size_t(abs_i / t.gather_slots) * size_t(t.gather_stride) + size_t(abs_i % t.gather_slots)],
                            t.src_start_us, t.src_air_us);
        t.tx_build[abs_i] = tx;
    } else if (t.gather_src) { // (batches only) gathered records
        tx = t.gather_src[size_t(abs_i / t.gather_slots) * size_t(t.gather_stride) + size_t(abs_i % t.gather_slots)];
        t.tx_build[abs_i] = tx;
    } else {
        tx = t.tx[abs_i];
    }
    if (t.check_span && tx.src >= 0 && (tx.start_us < t.span_begin || tx.start_us + tx.air_us > t.span_end))
        t.stage_count[6] = 1u; // reported as RM_ERR_STATE when the tick's result is read
    if (t.check_txprob && tx.src >= 0 && tx.txprob > 0.0 && tx.txprob < 1.0) t.stage_count[6] = 2u; // (as well)
    float4 f;
    double thr64;
    tx_prefilter(m, tx, f, thr64);
    if (t.nc.state != nullptr) { // (block-uniform) the source candidate cache: a frame whose source has a valid list is not swept
        uint2 h = make_uint2(0u, 0u);
        if (t.nc.arena_rssi != nullptr) {
            // heard form (block-uniform): the pool's entry, which another context's publish kernel may be storing right now on another
            // stream.  ONE 8-byte load: a value that is not the newest is an older one -- a miss, or a valid entry with its final
            // offset and length, whose records were written back before the kernel that stored it began (rm_engine.h).
            if (tx.src >= 0) {
                const uint64_t en = __hip_atomic_load(&t.nc.entry[tx.src], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (nc_entry_word(en) == t.nc.word) h = make_uint2(nc_entry_len(en) + 1u, nc_entry_off(en));
            }
        } else if (tx.src >= 0 && t.nc.state[tx.src] == t.nc.word) {
            h = make_uint2(t.nc.len[tx.src] + 1u, t.nc.off[tx.src]);
        }
        t.nc.hit[e] = h;
        const bool swept = h.x == 0u && f.w >= 0.f;
        if (h.x) f.w = -1.f; // (never near: the near-frame lists and phase A drop it)
        const uint64_t sm = ballot64(swept), hm = ballot64(h.x != 0u);
        const int lane = threadIdx.x & 63;
        if (sm && lane == __ffsll((long long)sm) - 1) atomicAdd(&t.nc.tick_cnt[0], uint32_t(__popcll(sm)));
        if (hm && lane == __ffsll((long long)hm) - 1) atomicAdd(&t.nc.tick_cnt[2], uint32_t(__popcll(hm)));
        // heard form (block-uniform): the tick's list of frames without a hit, the ones that reach nobody included -- what the
        // reorder stage walks and the claim and the fill look at.  One allocation per wave; the order among waves is the atomics'.
        if (t.nc.arena_rssi != nullptr) {
            const uint64_t um = ballot64(h.x == 0u);
            if (um) {
                const int first = __ffsll((long long)um) - 1;
                uint32_t base = 0;
                if (lane == first) base = atomicAdd(&t.nc.tick_cnt[3], uint32_t(__popcll(um)));
                base = uint32_t(__shfl(int(base), first));
                if (h.x == 0u) t.nc.unserved[base + lane_prefix(um)] = e;
            }
        }
    }
    const float inv = prefilter_inv(m, f);
    t.p_txf[e] = f;
    t.p_ch[e] = tx.channel;
    t.p_src[e] = tx.src;
    t.p_inv[e] = inv;
}

__global__ void __launch_bounds__(256) k_tick_prep(const NodesDev nd, const ModelDev m, const TickDev t)
{
    tick_prep_body(nd, m, t);
}

__global__ void __launch_bounds__(256) k_tick_prep_batch(const NodesDev nd, const ModelDev m, const TickDev *__restrict__ ticks)
{
    tick_prep_body(nd, m, ticks[blockIdx.z]);
}

// the receivers of a two-level filter workgroup (the same tiling for every tick of a launch: t is any of them); false: this
// wave has no slab
template <int RPT, bool SHADOW>
RM_D bool wg_rx_load(const NodesDev &nd, const TickDev &t, WgRx<RPT> &rx)
{
    const int lane = threadIdx.x & 63;
    const int wave = wave_index();
    const int wg = blockIdx.x;
    const int slab = wg * kWavesPerBlock + wave;
    const int jbase = slab * (kGroup * RPT);
    const bool live = slab < t.n_slabs;
    const int n_groups = (t.n_rx + kGroup - 1) / kGroup;
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int j = jbase + r * kGroup + lane;
        rx.fx[r] = rx.fy[r] = rx.fz[r] = __builtin_nanf("");
        rx.fch[r] = 0;
        rx.forig[r] = 0;
        if (live && j < t.n_rx) {
            const float4 v = nd.rxf[j];
            rx.fx[r] = v.x;
            rx.fy[r] = v.y;
            rx.fz[r] = v.z;
            rx.fch[r] = __float_as_int(v.w);
            if (SHADOW) rx.forig[r] = nd.orig[j];
        }
        const int g = slab * RPT + r;
        const bool ok = live && g * kGroup < t.n_rx;
        rx.bxy[r] = ok ? nd.bbox_xy[g] : make_float4(0.f, 0.f, 0.f, 0.f);
        rx.bz[r] = ok ? nd.bbox_z[g] : make_float2(0.f, 0.f);
        rx.bmask[r] = ok ? nd.grp_chmask[g] : 0u;
    }
    // union box of the workgroup's 4*RPT groups
    if (RPT == 4) {
        rx.w.xy = nd.wg_box_xy[wg];
        rx.w.z = nd.wg_box_z[wg];
        rx.w.chmask = nd.wg_chmask[wg];
    } else {
        rx.w = box_union_empty();
        for (int g = wg * kWavesPerBlock * RPT; g < min(n_groups, (wg + 1) * kWavesPerBlock * RPT); ++g) // uniform
            box_union_add(rx.w, nd.bbox_xy[g], nd.bbox_z[g], nd.grp_chmask[g]);
    }
    return live;
}

constexpr int kNearLds = 512; // near-frame records held in LDS between two phase-B rounds
constexpr int kUnrollA = 4;   // phase A works on kUnrollA x 256 frames at a time: their records are requested together

// LDS of a per-tick two-level filter workgroup: the near frames' records, the waves' candidate ballots, the link-hash table
template <int RPT, bool SHADOW> struct SweepLds {
    float4 txf[kNearLds];
    int ch[kNearLds];
    int e[kNearLds];
    float inv[SHADOW ? kNearLds : 1];
    int src[SHADOW ? kNearLds : 1];
    uint64_t mask[kWavesPerBlock][kTxChunk][RPT];
    uint32_t tbl[SHADOW ? kShadowBins : 1];
    uint32_t n;
};

// once per workgroup, before its first sweep
template <class Lds> RM_D void sweep_lds_init(Lds &L, const ModelDev &m, const bool shadow)
{
    if (shadow) L.tbl[threadIdx.x] = m.shadow_tbl[threadIdx.x]; // kBlock == kShadowBins
    if (threadIdx.x == 0) L.n = 0u;
    __syncthreads();
}

// One tick of the two-level filter for the receivers in `rx` (live: this wave has a slab); tick_salt spreads the ticks of a launch
// over the shards.  Phase A looks at all of the tick's frames, or (RPT == 4, large tables in batches) at the list of those near
// this workgroup's block of kNearSb workgroups.
template <int RPT, bool SHADOW>
RM_D void filter_wg_tick(const ModelDev &m, SweepLds<RPT, SHADOW> &L, const WgRx<RPT> &rx, const bool live, const TickDev &t, const uint32_t tick_salt)
{
    const int32_t *const near_list = (RPT == 4 && t.near_list) ? t.near_list + size_t(blockIdx.x / kNearSb) * size_t(t.near_cap) : nullptr;
    const int n_look = near_list ? uniform_i(int(min(t.near_cnt[blockIdx.x / kNearSb], uint32_t(t.near_cap)))) : t.n_active - t.first_eval;
    uint32_t round = 0; // phase-B chunks so far: spreads a wave's runs over the shards
    const int lane = threadIdx.x & 63;
    const int wave = wave_index();
    const int slab = blockIdx.x * kWavesPerBlock + wave;
    const int jbase = slab * (kGroup * RPT);
    for (int g0 = 0; g0 < n_look; g0 += kUnrollA * kBlock) { // block-uniform
        // the records of kUnrollA x 256 frames, requested together (one exposed round trip per 1024 frames)
        float4 af[kUnrollA];
        int ach[kUnrollA], asrc[kUnrollA], ae[kUnrollA];
        float ainv[kUnrollA];
#pragma unroll
        for (int u = 0; u < kUnrollA; ++u) {
            af[u] = make_float4(0.f, 0.f, 0.f, -1.f);
            ach[u] = 0;
            asrc[u] = -1;
            ainv[u] = 0.f;
            ae[u] = -1;
            const int i = g0 + u * kBlock + int(threadIdx.x);
            if (i < n_look) {
                const int e = near_list ? near_list[i] : i;
                ae[u] = e;
                af[u] = t.p_txf[e];
                ach[u] = t.p_ch[e];
                if (SHADOW) {
                    ainv[u] = t.p_inv[e];
                    asrc[u] = t.p_src[e];
                }
            }
        }
#pragma unroll 1
        for (int u = 0; u < kUnrollA; ++u) { // rolled: one copy of phase B; the records are selected, not indexed
            const int f0 = g0 + u * kBlock;
            if (f0 >= n_look) break; // block-uniform
            float4 tfa = af[0];
            int cha = ach[0], srca = asrc[0], e = ae[0];
            float inva = ainv[0];
#pragma unroll
            for (int k = 1; k < kUnrollA; ++k) {
                tfa.x = (u == k) ? af[k].x : tfa.x;
                tfa.y = (u == k) ? af[k].y : tfa.y;
                tfa.z = (u == k) ? af[k].z : tfa.z;
                tfa.w = (u == k) ? af[k].w : tfa.w;
                cha = (u == k) ? ach[k] : cha;
                srca = (u == k) ? asrc[k] : srca;
                inva = (u == k) ? ainv[k] : inva;
                e = (u == k) ? ae[k] : e;
            }
            // phase A: this thread's frame against the workgroup box (and: does anybody here listen on its channel)
            const bool hit = e >= 0 && box_near(rx.w.xy, rx.w.z, tfa) && ((rx.w.chmask >> (uint32_t(cha) & 31u)) & 1u) != 0u;
            const uint64_t hm = ballot64(hit);
            if (hm) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&L.n, uint32_t(__popcll(hm)));
                base = __builtin_amdgcn_readfirstlane(base);
                if (hit) {
                    const uint32_t k = base + lane_prefix(hm);
                    L.txf[k] = tfa;
                    L.ch[k] = cha;
                    L.e[k] = e;
                    if (SHADOW) {
                        L.inv[k] = inva;
                        L.src[k] = srca;
                    }
                }
            }
            __syncthreads();
            const int n_near = uniform_i(int(L.n));
            const bool last = f0 + kBlock >= n_look;
            if (!last && n_near + kBlock <= kNearLds) continue; // room for another 256 frames

            // phase B: chunks of 64 near frames, every wave for its own groups
            if (live) {
                for (int c0 = 0; c0 < n_near; c0 += kTxChunk) {
                    const Staged s{L.txf, L.ch, L.inv, L.src, L.tbl, nullptr, c0};
                    uint64_t near[RPT];
                    const uint64_t todo = near_groups(rx, s, min(kTxChunk, n_near - c0), slab, t.n_rx, lane, near);
                    // Pass 1, the reservation and pass 2 of sweep_two_pass with RunPerWave, as their own text: through the shared
                    // function this form's kernels need some ten scalar registers more, which costs k_filter_wg<4|2, true> a
                    // spill register and with it an occupancy step; the tests are the same expressions.
                    const int nt = min(kTxChunk, n_near - c0);
                    uint32_t my_total = 0;
                    uint64_t walk = todo;
                    while (walk) {
                        const int ti = __ffsll((long long)walk) - 1; // wave-uniform
                        walk &= walk - 1;
                        const float4 tf = L.txf[c0 + ti];
                        const int tch = L.ch[c0 + ti];
                        uint64_t mask[RPT];
                        uint32_t total = 0;
#pragma unroll
                        for (int q = 0; q < RPT; ++q) {
                            mask[q] = 0;
                            if ((near[q] >> ti) & 1ull) {
                                const float s2 = dist2_f32(rx.fx[q] - tf.x, rx.fy[q] - tf.y, rx.fz[q] - tf.z);
                                bool h = (s2 <= tf.w) && (rx.fch[q] == tch);
                                if (SHADOW && h) h = shadow_pass(m, L.tbl, s2, L.inv[c0 + ti], L.src[c0 + ti], rx.forig[q]);
                                mask[q] = ballot64(h);
                                total += uint32_t(__popcll(mask[q]));
                            }
                        }
                        if (total) {
                            if (lane == ti) my_total = total;
                            if (lane < RPT) {
                                uint64_t v = mask[0];
#pragma unroll
                                for (int q = 1; q < RPT; ++q) v = (lane == q) ? mask[q] : v;
                                L.mask[wave][ti][lane] = v;
                            }
                        }
                    }
                    const uint64_t have = ballot64(my_total != 0u);
                    if (have == 0) continue;
                    const int my_e = L.e[c0 + min(lane, nt - 1)];
                    if (!t.use_matrix && my_total != 0u && t.first_eval + my_e >= t.first_new) atomicAdd(&t.cand_tot[my_e - t.cnt_base], my_total);
                    const uint32_t inc = wave_inclusive_scan(my_total, lane);
                    const uint32_t wave_total = __shfl(inc, 63);
                    const uint32_t shard = (uint32_t(slab) + (round + uint32_t(c0 >> 6)) * 37u + tick_salt * 101u) & t.shard_mask;
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&t.shard_count[shard * kShardStride], wave_total);
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (base + wave_total > t.seg_cap) { // the shard is full: drop the run, flag the tick
                        if (lane == 0) t.stage_count[1] = 1u;
                        continue;
                    }
                    const uint32_t my_base = shard * t.seg_cap + base + inc - my_total;
                    walk = have;
                    while (walk) {
                        const int ti = __ffsll((long long)walk) - 1;
                        walk &= walk - 1;
                        const uint32_t fbase = __shfl(my_base, ti);
                        const int e_ti = L.e[c0 + ti];
                        uint32_t pre = 0;
#pragma unroll
                        for (int q = 0; q < RPT; ++q) {
                            const uint64_t mk = L.mask[wave][ti][q];
                            if (mk == 0) continue;
                            if ((mk >> lane) & 1ull) {
                                const uint32_t idx = fbase + pre + lane_prefix(mk);
                                t.st_pkt[idx] = e_ti;
                                t.st_dst[idx] = jbase + q * kGroup + lane;
                                if (t.use_matrix) t.st_blk[idx] = fbase;
                            }
                            pre += uint32_t(__popcll(mk));
                        }
                    }
                }
            }
            round += uint32_t(kNearLds / kTxChunk);
            __syncthreads(); // every wave is done with the LDS records
            if (threadIdx.x == 0) L.n = 0u;
            __syncthreads();
            if (last) break;
        }
    }
}

// the source candidate cache served every frame of these ticks: nothing is left for the sweep (block-uniform)
RM_D bool nc_nothing_to_sweep(const TickDev *__restrict__ ticks, const int first, const int count)
{
    if (ticks[first].nc.state == nullptr) return false;
    for (int b = 0; b < count; ++b)
        if (uniform_u(ticks[first + b].nc.tick_cnt[0]) != 0u) return false;
    return true;
}

// `ticks[first .. first + count)`: the ticks this workgroup sweeps one after the other against ITS receivers, which stay
// in registers (and their boxes) for all of them -- at a million receivers the 16 MB of pre-filter records then leave HBM
// once per `count` ticks instead of once per tick.
template <int RPT, bool SHADOW>
RM_D void filter_wg_body(const NodesDev &nd, const ModelDev &m, const TickDev *__restrict__ ticks, const int first, const int count)
{
    __shared__ SweepLds<RPT, SHADOW> L;
    if (nc_nothing_to_sweep(ticks, first, count)) return;
    WgRx<RPT> rx;
    const bool live = wg_rx_load<RPT, SHADOW>(nd, ticks[first], rx);
    sweep_lds_init(L, m, SHADOW);
    for (int b = 0; b < count; ++b) {
        if (nc_nothing_to_sweep(ticks, first + b, 1)) continue; // (block-uniform)
        filter_wg_tick<RPT, SHADOW>(m, L, rx, live, ticks[first + b], uint32_t(first + b));
    }
}

template <int RPT, bool SHADOW>
__global__ void __launch_bounds__(kBlock, RPT == 4 ? 4 : (RPT == 2 ? 5 : 6)) k_filter_wg(const NodesDev nd, const ModelDev m, const TickDev t)
{
    filter_wg_body<RPT, SHADOW>(nd, m, &t, 0, 1);
}

template <int RPT, bool SHADOW>
__global__ void __launch_bounds__(kBlock, 6)
k_filter_wg_batch(const NodesDev nd, const ModelDev m, const TickDev *__restrict__ ticks, const int n_ticks, const int per_wg)
{
    const int first = int(blockIdx.z) * per_wg;
    filter_wg_body<RPT, SHADOW>(nd, m, ticks, first, min(per_wg, n_ticks - first));
}

// The batch filter over the near-frame lists, SIXTEEN ticks at a time (RPT == 4: the large tables the lists are made for).
// With the lists a workgroup's phase A has a few dozen frames per tick to look at -- a few lanes of one round -- and what a
// tick cost was what every tick costs whatever its size: three dependent round trips (list length -> list entry -> record),
// three workgroup barriers and some eighty wave instructions of loop and bookkeeping per wave, 977 workgroups x 128 ticks of
// them per launch at a million receivers (two thirds of the filter's time there).  Here a wave asks for the lists of FOUR ticks
// per round (one per unrolled request: its lanes are the list's entries) and the workgroup's four waves for sixteen; the near
// frames of all of them are compacted into the same LDS list with their tick beside them, and phase B runs over full chunks of
// 64 near frames of mixed ticks: a frame's candidates go to ITS tick's shards (one allocation per frame and wave, by the lane
// the frame sits in), through its tick's descriptor.  The tests are filter_wg_tick's, expression for expression; the order of
// the candidates inside a tick's shards never mattered (the reorder stage sorts).
constexpr int kGrpTicks = 4 * kWavesPerBlock;

template <bool SHADOW>
__global__ void __launch_bounds__(kBlock, SHADOW ? 5 : 6)
k_filter_wg_group(const NodesDev nd, const ModelDev m, const TickDev *__restrict__ ticks, const int n_ticks, const int per_wg)
{
    constexpr int RPT = 4;
    __shared__ float4 s_txf[kNearLds];
    __shared__ int s_ch[kNearLds];
    __shared__ int s_e[kNearLds];
    __shared__ uint16_t s_tk[kNearLds]; // the frame's tick (index into `ticks`: at most RM_MAX_BATCH)
    __shared__ float s_inv[SHADOW ? kNearLds : 1];
    __shared__ int s_src[SHADOW ? kNearLds : 1];
    __shared__ uint64_t s_mask[kWavesPerBlock][kTxChunk][RPT];
    __shared__ uint32_t s_tbl[SHADOW ? kShadowBins : 1];
    __shared__ uint32_t s_n;

    const int first = int(blockIdx.z) * per_wg, count = min(per_wg, n_ticks - first);
    const int lane = threadIdx.x & 63;
    const int wave = wave_index();
    const int wg = blockIdx.x;
    const int sb = wg / kNearSb;
    const int slab = wg * kWavesPerBlock + wave;
    const int jbase = slab * (kGroup * RPT);
    if (nc_nothing_to_sweep(ticks, first, count)) return;
    WgRx<RPT> rx;
    wg_rx_load<RPT, SHADOW>(nd, ticks[first], rx); // (the receiver tiling is the same for every tick of a launch)
    const bool live = slab < ticks[first].n_slabs;
    const int n_rx = ticks[first].n_rx;
    const float (&fx)[RPT] = rx.fx, (&fy)[RPT] = rx.fy, (&fz)[RPT] = rx.fz;
    const int (&fch)[RPT] = rx.fch, (&forig)[RPT] = rx.forig;
    const float4 (&bxy)[RPT] = rx.bxy;
    const float2 (&bz)[RPT] = rx.bz;
    const float4 wxy = rx.w.xy;
    const float2 wz = rx.w.z;
    const uint32_t (&bmask)[RPT] = rx.bmask;
    const uint32_t wmask = rx.w.chmask;

    if (SHADOW) s_tbl[threadIdx.x] = m.shadow_tbl[threadIdx.x];
    if (threadIdx.x == 0) s_n = 0u;
    __syncthreads();

    uint32_t round = 0;
    for (int b0 = 0; b0 < count; b0 += kGrpTicks) { // block-uniform
        const int g = min(kGrpTicks, count - b0);
        // the lists' lengths (every wave reads all sixteen: nothing to agree on through LDS)
        int cnt_l = 0;
        if (lane < g) {
            const TickDev &T = ticks[first + b0 + lane];
            cnt_l = int(min(T.near_cnt[sb], uint32_t(T.near_cap)));
        }
        const int rounds = (uniform_i(wave_max_i(cnt_l)) + 63) >> 6;
        constexpr int kUnrollA = 4;
        float4 af[kUnrollA];
        int ach[kUnrollA], asrc[kUnrollA], ae[kUnrollA];
        float ainv[kUnrollA];
        for (int r = 0; r < rounds; ++r) { // block-uniform
#pragma unroll
            for (int u = 0; u < kUnrollA; ++u) { // this wave's tick of request u: u * 4 + wave
                const int tb = u * kWavesPerBlock + wave;
                const int c = uniform_i(__shfl(cnt_l, tb));
                const int k = (r << 6) + lane;
                af[u] = make_float4(0.f, 0.f, 0.f, -1.f);
                ach[u] = 0;
                asrc[u] = -1;
                ainv[u] = 0.f;
                ae[u] = -1;
                if (k < c) {
                    const TickDev &T = ticks[first + b0 + tb];
                    const int e = T.near_list[size_t(sb) * size_t(T.near_cap) + size_t(k)];
                    ae[u] = e;
                    af[u] = T.p_txf[e];
                    ach[u] = T.p_ch[e];
                    if (SHADOW) {
                        ainv[u] = T.p_inv[e];
                        asrc[u] = T.p_src[e];
                    }
                }
            }
#pragma unroll 1
            for (int u = 0; u < kUnrollA; ++u) { // rolled: one copy of phase B; the records are selected, not indexed
                if (u * kWavesPerBlock >= g) break; // block-uniform
                float4 tfa = af[0];
                int cha = ach[0], srca = asrc[0], e = ae[0];
                float inva = ainv[0];
#pragma unroll
                for (int k = 1; k < kUnrollA; ++k) {
                    tfa.x = (u == k) ? af[k].x : tfa.x;
                    tfa.y = (u == k) ? af[k].y : tfa.y;
                    tfa.z = (u == k) ? af[k].z : tfa.z;
                    tfa.w = (u == k) ? af[k].w : tfa.w;
                    cha = (u == k) ? ach[k] : cha;
                    srca = (u == k) ? asrc[k] : srca;
                    inva = (u == k) ? ainv[k] : inva;
                    e = (u == k) ? ae[k] : e;
                }
                // phase A: this thread's frame against the workgroup box
                bool hit = false;
                if (e >= 0) {
                    hit = box_near(wxy, wz, tfa) && ((wmask >> (uint32_t(cha) & 31u)) & 1u) != 0u; // (nobody here listens on its channel)
                }
                const uint64_t hm = ballot64(hit);
                if (hm) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&s_n, uint32_t(__popcll(hm)));
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (hit) {
                        const uint32_t k = base + lane_prefix(hm);
                        s_txf[k] = tfa;
                        s_ch[k] = cha;
                        s_e[k] = e;
                        s_tk[k] = uint16_t(first + b0 + u * kWavesPerBlock + wave);
                        if (SHADOW) {
                            s_inv[k] = inva;
                            s_src[k] = srca;
                        }
                    }
                }
                __syncthreads();
                const int n_near = uniform_i(int(s_n));
                const bool last = r + 1 >= rounds && (u + 1 >= kUnrollA || (u + 1) * kWavesPerBlock >= g);
                if (!last && n_near + kBlock <= kNearLds) continue; // room for another 256 frames

                // phase B: chunks of 64 near frames (of any of the group's ticks), every wave for its own groups
                if (live) {
                    for (int c0 = 0; c0 < n_near; c0 += kTxChunk) {
                        const int nt = min(kTxChunk, n_near - c0);
                        uint64_t near[RPT];
                        uint64_t todo = 0;
                        {
                            const float4 tf = s_txf[c0 + min(lane, nt - 1)];
                            const uint32_t tchb = uint32_t(s_ch[c0 + min(lane, nt - 1)]) & 31u;
#pragma unroll
                            for (int q = 0; q < RPT; ++q) {
                                near[q] = 0;
                                if ((slab * RPT + q) * kGroup < n_rx) {
                                    near[q] = ballot64(lane < nt && box_near(bxy[q], bz[q], tf) && ((bmask[q] >> tchb) & 1u) != 0u);
                                }
                                todo |= near[q];
                            }
                        }
                        uint32_t my_total = 0;
                        uint64_t walk = todo;
                        while (walk) {
                            const int ti = __ffsll((long long)walk) - 1; // wave-uniform
                            walk &= walk - 1;
                            const float4 tf = s_txf[c0 + ti];
                            const int tch = s_ch[c0 + ti];
                            uint64_t mask[RPT];
                            uint32_t total = 0;
#pragma unroll
                            for (int q = 0; q < RPT; ++q) {
                                mask[q] = 0;
                                if ((near[q] >> ti) & 1ull) {
                                    const float s2 = dist2_f32(fx[q] - tf.x, fy[q] - tf.y, fz[q] - tf.z);
                                    bool h = (s2 <= tf.w) && (fch[q] == tch);
                                    if (SHADOW && h) {
                                        h = shadow_pass(m, s_tbl, s2, s_inv[c0 + ti], s_src[c0 + ti], forig[q]);
                                    }
                                    mask[q] = ballot64(h);
                                    total += uint32_t(__popcll(mask[q]));
                                }
                            }
                            if (total) {
                                if (lane == ti) my_total = total;
                                if (lane < RPT) {
                                    uint64_t v = mask[0];
#pragma unroll
                                    for (int q = 1; q < RPT; ++q) v = (lane == q) ? mask[q] : v;
                                    s_mask[wave][ti][lane] = v;
                                }
                            }
                        }
                        uint64_t have = ballot64(my_total != 0u);
                        if (have == 0) continue;
                        // the lane of a frame with candidates: its tick's counters and shards
                        uint32_t my_base = 0;
                        if (my_total != 0u) {
                            const int my_e = s_e[c0 + lane];
                            const int my_tk = int(s_tk[c0 + lane]);
                            const TickDev &T = ticks[my_tk];
                            if (!T.use_matrix && T.first_eval + my_e >= T.first_new) atomicAdd(&T.cand_tot[my_e - T.cnt_base], my_total);
                            const uint32_t shard = (uint32_t(slab) + (round + uint32_t(c0 >> 6)) * 37u + uint32_t(my_tk) * 101u + uint32_t(lane) * 7u) & T.shard_mask;
                            const uint32_t base = atomicAdd(&T.shard_count[shard * kShardStride], my_total);
                            if (base + my_total > T.seg_cap) { // the shard is full: drop the run, flag the tick
                                T.stage_count[1] = 1u;
                                my_total = 0u;
                            }
                            my_base = shard * T.seg_cap + base;
                        }
                        have = ballot64(my_total != 0u);
                        walk = have;
                        while (walk) {
                            const int ti = __ffsll((long long)walk) - 1;
                            walk &= walk - 1;
                            const uint32_t fbase = uniform_u(uint32_t(__shfl(int(my_base), ti)));
                            const int e_ti = s_e[c0 + ti];
                            const TickDev &T = ticks[uniform_i(int(s_tk[c0 + ti]))];
                            uint32_t pre = 0;
#pragma unroll
                            for (int q = 0; q < RPT; ++q) {
                                const uint64_t mk = s_mask[wave][ti][q];
                                if (mk == 0) continue;
                                if ((mk >> lane) & 1ull) {
                                    const uint32_t idx = fbase + pre + lane_prefix(mk);
                                    T.st_pkt[idx] = e_ti;
                                    T.st_dst[idx] = jbase + q * kGroup + lane;
                                    if (T.use_matrix) T.st_blk[idx] = fbase; // the run's base: only the ordered scatter of unsorted tables ranks inside it
                                }
                                pre += uint32_t(__popcll(mk));
                            }
                        }
                    }
                }
                round += uint32_t(kNearLds / kTxChunk);
                __syncthreads(); // every wave is done with the LDS records
                if (threadIdx.x == 0) s_n = 0u;
                __syncthreads();
                if (last) break;
            }
        }
    }
}

// The near-frame lists of a batch over a large table (blockIdx.x = block of kNearSb filter workgroups, blockIdx.z = tick): at
// a million receivers a tick has a thousand filter workgroups, and every one of them reading and testing every frame of the
// tick was 27 MB of L2 reads per tick and a third of the filter's time; a block's box (16 k receivers) is near to a few
// dozen of a thousand frames, and its workgroups look at those.
__global__ void __launch_bounds__(256) k_near_lists(const NodesDev nd, const TickDev *__restrict__ ticks, const int n_wg)
{
    __shared__ BoxUnion s_box;
    __shared__ uint32_t s_n;
    const TickDev &t = ticks[blockIdx.z];
    const int sb = blockIdx.x, lane = threadIdx.x & 63;
    const int n_eval = t.n_active - t.first_eval;
    if (t.near_list == nullptr) return;
    // the source cache's heard form, a tick that left no frame to the sweep (block-uniform, as nc_nothing_to_sweep below): no
    // frame is near to anything, the lists are empty
    if (t.nc.arena_rssi != nullptr && uniform_u(t.nc.tick_cnt[0]) == 0u) {
        if (threadIdx.x == 0) const_cast<uint32_t *>(t.near_cnt)[sb] = 0u;
        return;
    }
    if (threadIdx.x < 64) { // the union of the block's workgroup boxes and channel masks
        const int w = sb * kNearSb + lane;
        BoxUnion u = box_union_empty();
        if (lane < kNearSb && w < n_wg) box_union_add(u, nd.wg_box_xy[w], nd.wg_box_z[w], nd.wg_chmask[w]);
        box_union_lanes(u, kNearSb / 2);
        if (threadIdx.x == 0) {
            s_box = u;
            s_n = 0u;
        }
    }
    __syncthreads();
    const BoxUnion box = s_box;
    int32_t *const list = const_cast<int32_t *>(t.near_list) + size_t(sb) * size_t(t.near_cap);
    for (int e0 = 0; e0 < n_eval; e0 += 256) { // block-uniform
        const int e = e0 + int(threadIdx.x);
        bool hit = false;
        if (e < n_eval) {
            const float4 f = t.p_txf[e];
            const uint32_t ch = uint32_t(t.p_ch[e]) & 31u;
            hit = box_near(box.xy, box.z, f) && ((box.chmask >> ch) & 1u) != 0u; // (the workgroups' own test, against the larger box)
        }
        const uint64_t hm = ballot64(hit);
        if (hm) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&s_n, uint32_t(__popcll(hm)));
            base = uniform_u(base);
            if (hit) list[base + lane_prefix(hm)] = e;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) const_cast<uint32_t *>(t.near_cnt)[sb] = s_n;
    // (Padding the list to the next 1024 entries with -1, so that phase A can ask for its entries before it knows the length --
    // one round trip less per workgroup and tick -- was measured: 255 instead of 220 us per 64 ticks at a million receivers,
    // the three extra loads per thread cost more than the round trip.)
}

// ============================================================================ launchers and planner

// Chooses the filter variant for this tick and fixes the receiver tiling (t.rpt, t.n_slabs):
//  kFilterGrid: k_filter on a (slab, tile) grid -- the general variant (fp64 frame, unsorted tables);
//  kFilterWg:   k_tick_prep + k_filter_wg, two-level cull inside one workgroup per 4*rpt groups.
PlanKnobs read_plan_knobs()
{
    PlanKnobs k{0, 0, false, 0};
    if (const char *e = getenv("RM_FILTER")) {
        if (!strcmp(e, "grid")) k.filter = kFilterGrid + 1;
        else if (!strcmp(e, "wg")) k.filter = kFilterWg + 1;
    }
    if (const char *e = getenv("RM_WG_RPT")) k.wg_rpt = (atoi(e) == 4) ? 4 : (atoi(e) == 2 ? 2 : 1);
    k.no_shadow_table = getenv("RM_NO_SHADOW_TABLE") != nullptr;
    return k;
}

int plan_filter(TickDev &t, const LaunchCfg &cfg, bool want_wg, const PlanKnobs &knobs)
{
    const int n_eval = t.n_active - t.first_eval;
    const int n_chunks = cdiv(max(n_eval, 1), kTxChunk);
    const long waves4 = long(cdiv(t.n_rx, 256)) * n_chunks;
    // enough waves to fill 256 CUs x 4 SIMDs several times over, else one group per wave
    t.rpt = (waves4 >= 4096) ? 4 : 1;
    t.n_slabs = cdiv(t.n_rx, 64 * t.rpt);
    int mode = kFilterGrid;
    if (cfg.bbox && !cfg.f64_filter) {
        const long pairs = long((cdiv(t.n_slabs, kWavesPerBlock) + 7) / 8 * 8) * n_chunks;
        // beyond a few thousand (workgroup, tile) pairs the 2-D grid of k_filter is mostly short-lived
        // workgroups that find nothing (1 M nodes, or thousands of frames on the air)
        if (t.rpt == 4 && pairs > 8192 && t.n_slabs >= 4 * 256) mode = kFilterWg;
        if (knobs.filter) mode = knobs.filter - 1;
        if (want_wg) mode = kFilterWg;
        if (mode == kFilterWg) {
            // batches bring their own parallelism (workgroups x ticks): the coarse tiling halves the frame x
            // workgroup-box tests of phase A twice over; a lone tick needs the workgroups
            // (a receiver partition's few tiles per tick are enough when the batch has hundreds of ticks: 13 workgroups x 256)
            int rpt = (t.n_rx > 400000 || (want_wg && (t.n_rx >= 16384 || long(t.n_rx) * knobs.batch_ticks >= (1L << 20)))) ? 4 : 1;
            if (knobs.wg_rpt) rpt = knobs.wg_rpt;
            t.rpt = rpt;
            t.n_slabs = cdiv(t.n_rx, 64 * t.rpt);
        }
    }
    t.filter_mode = mode;
    return mode;
}

hipError_t launch_filter(hipStream_t s, const NodesDev &nd, const ModelDev &m, const TickDev &t,
                         const LaunchCfg &cfg)
{
    const int n_eval = t.n_active - t.first_eval;
    if (n_eval <= 0 || t.n_slabs <= 0) return hipSuccess;
    if (t.filter_mode == kFilterWg) {
        RM_KLAUNCH(k_tick_prep, dim3(cdiv(n_eval, 256)), dim3(256), 0, s, nd, m, t);
        const dim3 grid(cdiv(t.n_slabs, kWavesPerBlock)), block(kBlock);
        if (t.rpt == 4) {
            if (cfg.shadow) RM_KLAUNCH((k_filter_wg<4, true>), grid, block, 0, s, nd, m, t);
            else RM_KLAUNCH((k_filter_wg<4, false>), grid, block, 0, s, nd, m, t);
        } else if (t.rpt == 2) {
            if (cfg.shadow) RM_KLAUNCH((k_filter_wg<2, true>), grid, block, 0, s, nd, m, t);
            else RM_KLAUNCH((k_filter_wg<2, false>), grid, block, 0, s, nd, m, t);
        } else {
            if (cfg.shadow) RM_KLAUNCH((k_filter_wg<1, true>), grid, block, 0, s, nd, m, t);
            else RM_KLAUNCH((k_filter_wg<1, false>), grid, block, 0, s, nd, m, t);
        }
        return hipGetLastError();
    }
    // XCD-aware launch: workgroups are dealt round-robin over the 8 XCDs in linear order (x fastest),
    // so with gridDim.x a multiple of 8 every tile-workgroup of one receiver slab has the same
    // blockIdx.x % 8 -- one XCD, one L2 -- and the slab's records leave HBM once per tick, not once
    // per XCD (placement is a speed matter only; the padding workgroups exit at once)
    const dim3 grid((cdiv(t.n_slabs, kWavesPerBlock) + 7) / 8 * 8, cdiv(n_eval, kTxChunk));
    const dim3 block(kBlock);
#define RM_LAUNCH(RPT, F64, BBOX, SH) RM_KLAUNCH((k_filter<RPT, F64, BBOX, SH>), grid, block, 0, s, nd, m, t)
    if (t.rpt == 4) {
        if (cfg.f64_filter) RM_LAUNCH(4, true, false, false);
        else if (cfg.bbox && cfg.shadow) RM_LAUNCH(4, false, true, true);
        else if (cfg.bbox) RM_LAUNCH(4, false, true, false);
        else if (cfg.shadow) RM_LAUNCH(4, false, false, true);
        else RM_LAUNCH(4, false, false, false);
    } else {
        if (cfg.f64_filter) RM_LAUNCH(1, true, false, false);
        else if (cfg.bbox && cfg.shadow) RM_LAUNCH(1, false, true, true);
        else if (cfg.bbox) RM_LAUNCH(1, false, true, false);
        else if (cfg.shadow) RM_LAUNCH(1, false, false, true);
        else RM_LAUNCH(1, false, false, false);
    }
#undef RM_LAUNCH
    return hipGetLastError();
}

// ticks of a batch a filter workgroup sweeps with ONE load of its receivers (rm_batch_tile_reuse reports it: the receiver
// table leaves HBM once per that many ticks of a launch)
int filter_ticks_per_wg(const TickDev &t0, int n)
{
    const int tiles = cdiv(t0.n_slabs, kWavesPerBlock);
    int per_wg = max(1, min(n, (tiles * n) / 3072));
    if (const char *e = getenv("RM_FILTER_TICKS_PER_WG")) per_wg = max(1, min(n, atoi(e)));
    return per_wg;
}

// rm_batch_*, stage 0: every tick's pre-pass and two-level filter (blockIdx.z = tick); `ticks` are the host
// copies of the descriptors (grid sizes), `b` the same descriptors in device memory
hipError_t launch_filter_batch(hipStream_t s, const NodesDev &nd, const ModelDev &m, const TickDev *ticks, int n, const TickDev *b,
                               const LaunchCfg &cfg)
{
    int max_eval = 0;
    for (int i = 0; i < n; ++i) max_eval = max(max_eval, ticks[i].n_active - ticks[i].first_eval);
    const TickDev &t0 = ticks[0];
    if (t0.n_pub <= 0) // (a rank's frame lists: k_rank_frames was this batch's pre-pass as well)
        RM_KLAUNCH(k_tick_prep_batch, dim3(cdiv(max_eval, 256), 1, n), dim3(256), 0, s, nd, m, b);
    if (t0.near_list != nullptr) { // (every tick of the batch has its lists, or none has)
        const int n_wg = cdiv(t0.n_rx, kGroup * 16);
        RM_KLAUNCH(k_near_lists, dim3(cdiv(n_wg, kNearSb), 1, n), dim3(256), 0, s, nd, b, n_wg);
    }
    // A workgroup keeps its receivers for `per_wg` ticks: as many as leave a few thousand workgroups for the chip (a table
    // of a million receivers has a thousand tiles: 16 ticks = 4 per workgroup; 100 k receivers: one tick per workgroup).
    const int tiles = cdiv(t0.n_slabs, kWavesPerBlock);
    const int per_wg = filter_ticks_per_wg(t0, n);
    const dim3 grid(tiles, 1, cdiv(n, per_wg)), block(kBlock);
    // The lists of sixteen ticks at a time pay where a list is a few dozen frames -- many blocks (a million receivers), or few
    // frames for this partition's part of the plane; with lists of hundreds of frames (configs[2] / [3] at 100 k receivers: seven
    // blocks) a round of the per-tick form is already full and the grouped one was measured 6 % / 13 % slower.
    // RM_FILTER_GROUP=0 / 1: never / whenever the launch allows it (read per launch: tests).
    const char *e_grp = getenv("RM_FILTER_GROUP");
    const int n_sb = cdiv(tiles, kNearSb);
    const double seen = double(max_eval) * fmin(1.0, 1.3 * double(t0.n_rx) / double(max(nd.n, 1)) + 0.02); // frames this partition keeps
    bool group = n_sb >= 32 || seen * 1.5 / double(n_sb) <= 128.0;
    if (e_grp) group = atoi(e_grp) != 0;
    if (t0.rpt == 4 && t0.near_list != nullptr && per_wg > 1 && group) {
        if (cfg.shadow) RM_KLAUNCH((k_filter_wg_group<true>), grid, block, 0, s, nd, m, b, n, per_wg);
        else RM_KLAUNCH((k_filter_wg_group<false>), grid, block, 0, s, nd, m, b, n, per_wg);
    } else if (t0.rpt == 4) {
        if (cfg.shadow) RM_KLAUNCH((k_filter_wg_batch<4, true>), grid, block, 0, s, nd, m, b, n, per_wg);
        else RM_KLAUNCH((k_filter_wg_batch<4, false>), grid, block, 0, s, nd, m, b, n, per_wg);
    } else if (t0.rpt == 2) {
        if (cfg.shadow) RM_KLAUNCH((k_filter_wg_batch<2, true>), grid, block, 0, s, nd, m, b, n, per_wg);
        else RM_KLAUNCH((k_filter_wg_batch<2, false>), grid, block, 0, s, nd, m, b, n, per_wg);
    } else {
        if (cfg.shadow) RM_KLAUNCH((k_filter_wg_batch<1, true>), grid, block, 0, s, nd, m, b, n, per_wg);
        else RM_KLAUNCH((k_filter_wg_batch<1, false>), grid, block, 0, s, nd, m, b, n, per_wg);
    }
    return hipGetLastError();
}

} // namespace rm
