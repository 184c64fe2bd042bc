// rm_ccabatch.hip -- the gate of a carrier-sense gated BATCH (rm_batch_run_sources_cca*)
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math)
//
// Candidate i of tick b is sensed (E5, at the tick's sample time, on its own channel) over the frames of the on-air window plus the
// KEPT frames of ticks 0 .. b-1 of the batch; it is kept iff its flags are 0.  Whether a frame of tick b-1 is on the air depends on
// tick b-1's gate: a serial chain -- in the DECISION only.  Which frame can be sensed by which candidate, and with what power, depends
// on positions, channels, times and the link hash, not on who deferred.  So:
//   k_ccab_begin     the ticks' descriptors from the host's pinned block into device memory, the index's counters to zero.
//   k_ccab_index     one thread per frame -- the window's records, then the records of ALL candidates as if kept (built here with
//                    make_tx_record, into a scratch array) -- into the query's kind of index: a kEdG x kEdG grid over the fp32 frame,
//                    kCbK entries per cell, the rest in the EVERY list; every frame also joins its source node's chain.
//   k_ccab_pairs     one WAVE per candidate of any tick (k_cca_gate's walk).  A frame counts for a candidate of tick b if it is a
//                    window frame or a frame of a tick b' < b, and is live at tick b's sample time.  <FILL = false>: counts the batch
//                    frames that pass the conservative tests -- an upper bound of the candidate's pairs.  <FILL = true>: evaluates
//                    (fp64, Q80) with full lanes; window frames are added into the candidate's 128-bit base sum, batch frames are
//                    appended as (frame, term) pairs to its segment.  A frame of the candidate's own node that spans the sample is
//                    RM_ED_TRANSMITTING at once (window) or a pair with bit 31 set (batch: only if that frame was kept).
//   k_ccab_scan_*    the counts' exclusive prefix = the segments (workgroup sums, their prefix, the workgroups' own prefixes); the total
//                    goes to the host, which sizes the buffer.
//   k_ccab_resolve   ONE workgroup walks the ticks in order, a thread per candidate: base sum + the terms of the pairs whose frame's
//                    kept bit is set (integer adds: the order cannot matter), 10 log10(sum + noise), flags, the kept bit, the gated
//                    list entry and the caller's outputs; __syncthreads() between ticks.  No grid-wide barrier anywhere.
// The sums are the exact Q80 integers of the lone gate, so a gated batch equals the same ticks as lone gated ticks bit for bit.
#include "rm_device.hpp"

namespace rm {

constexpr int kCbResolve = 1024; // threads of the one workgroup that resolves, and of a workgroup of the scan

__global__ void __launch_bounds__(256) k_ccab_begin(const CcaTick *h_ticks, int n_ticks, CcaTick *d_ticks, uint32_t *cnt, int cnt_len)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ticks) d_ticks[i] = h_ticks[i];
    if (i < cnt_len) cnt[i] = 0u;
}

template <bool GRID>
__global__ void __launch_bounds__(256) k_ccab_index(const NodesDev nd, const ModelDev m, const CcaBatchDev cb)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= cb.n_win + cb.n_cand) return;
    rm_tx_record r;
    int tk = -1;
    if (f < cb.n_win) {
        r = cb.win[f];
        cb.fr_tick[f] = -1;
        // a window frame that is live at neither the earliest nor any later sample of the batch has nothing to say
        if (r.src < 0 || r.start_us > cb.t_hi || !(cb.t_lo < r.start_us || cb.t_lo - r.start_us < r.air_us)) return;
    } else {
        const int s = f - cb.n_win;
        int lo = 0, hi = cb.n_ticks - 1; // the last tick whose first candidate is <= s (empty ticks before it share its offset)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cb.ticks[mid].first <= s) lo = mid;
            else hi = mid - 1;
        }
        tk = lo;
        const CcaTick t = cb.ticks[tk];
        const int j = t.src[s - t.first];
        r = make_tx_record(nd, j, t.start_us, t.air_us); // (an entry outside 0 .. n-1: a padding record)
        cb.scr[s] = r;
        cb.cand[s] = r.src;
        cb.fr_tick[f] = tk;
        if (r.src < 0) return;
    }
    cb_index_frame<GRID>(nd, m, cb, f, r, tk);
}

template <bool GRID, bool FILL>
__global__ void __launch_bounds__(256) k_ccab_pairs(const NodesDev nd, const ModelDev m, const CcaBatchDev cb)
{
    __shared__ uint32_t s_tbl[kShadowBins];
    __shared__ int s_off[kWavesPerBlock][65];
    __shared__ int s_cell[kWavesPerBlock][64];
    __shared__ int64_t s_start[kMaxBatch], s_air[kMaxBatch]; // the ticks' frames: one start and one air time per tick
    __shared__ uint32_t s_np[kWavesPerBlock];                // pairs the wave has appended

    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const bool shadow = m.shadow_tbl != nullptr;
    s_tbl[tid] = shadow ? m.shadow_tbl[tid] : 0xFFFFFFFFu;
    for (int b = tid; b < cb.n_ticks; b += kBlock) {
        s_start[b] = cb.ticks[b].start_us;
        s_air[b] = cb.ticks[b].air_us;
    }
    if (tid < kWavesPerBlock) s_np[tid] = 0u;
    __syncthreads();
    const int i = blockIdx.x * kWavesPerBlock + wave; // wave-uniform
    if (i >= cb.n_cand) return;
    const int j = uniform_i(cb.cand[i]);
    if (j < 0) { // padding has no pairs
        if (lane == 0) {
            if (FILL) cb.pair_fill[i] = 0u;
            else cb.pair_cnt[i] = 0u;
        }
        return;
    }
    const int b = uniform_i(cb.fr_tick[cb.n_win + i]);
    const int64_t t = cb.ticks[b].cca_us;
    const SrcRecord sr = nd.srec[j];
    const double rx_ = sr.x - m.org_x, ry_ = sr.y - m.org_y, rz_ = sr.z - m.org_z;
    const float px = float(rx_), py = float(ry_), pz = float(rz_);
    const bool wide = !(fabs(rx_) <= m.coord_bound && fabs(ry_) <= m.coord_bound && fabs(rz_) <= m.coord_bound);
    const EdNode nv{true, wide, shadow, sr.channel, j, px, py, pz};
    const uint32_t seg = FILL ? cb.pair_off[i] : 0u, cap = FILL ? cb.pair_off[i + 1] - seg : 0u;

    U128 acc = {0ull, 0ull};
    uint32_t n_cond = 0u; // (counting pass) batch frames that pass the conservative tests
    uint32_t tx = 0u;
    auto append = [&](const uint32_t slot, const U128 q) {
        const uint32_t at = atomicAdd(&s_np[wave], 1u);
        if (at < cap) {
            cb.pair_slot[seg + at] = slot;
            cb.pair_term[seg + at] = make_ulonglong2(q.lo, q.hi);
        } else {
            cb.h_info[1] = 1u; // (the counting pass applied the same tests to the same frames: its bound holds)
        }
    };
    auto look = [&](const float4 &p, const int4 &fm, const int tk) {
        if (!ed_candidate(m, s_tbl, nv, p, fm)) return;
        const bool batch = tk >= 0;
        if (batch && !(tk < b && cb_live(t, s_start[tk], s_air[tk]))) return;
        const rm_tx_record &w = batch ? cb.scr[fm.y - cb.n_win] : cb.win[fm.y];
        if (!batch && !cb_live(t, w.start_us, w.air_us)) return;
        if (!FILL) {
            n_cond += batch ? 1u : 0u;
            return;
        }
        const double rssi = logdist_rssi(m, w, sr.x, sr.y, sr.z, j);
        if (!(rssi >= m.ld_ifloor)) return;
        const U128 q = q80_from_double(det_pow10(rssi / 10.0));
        if (batch) append(uint32_t(fm.y - cb.n_win), q);
        else acc = u128_add(acc, q);
    };

    cb_walk<GRID>(cb, s_off[wave], s_cell[wave], lane, wide, px, py, look);

    // the node's own frames (its chain): a window frame that spans the sample says RM_ED_TRANSMITTING now, a frame of an earlier tick
    // of the batch says it if that frame was kept -- on any channel, whatever its reach
    if (lane == 0) {
        const unsigned long long head = cb.self_slot[j];
        int f = (uint32_t(head >> 32) == cb.stamp) ? int(uint32_t(head)) : -1;
        const U128 zero = {0ull, 0ull};
        while (f >= 0) {
            const int tk = cb.fr_tick[f];
            if (tk < 0) {
                if (cb_live(t, cb.win[f].start_us, cb.win[f].air_us)) tx = uint32_t(RM_ED_TRANSMITTING);
            } else if (tk < b && cb_live(t, s_start[tk], s_air[tk])) {
                if (FILL) append(uint32_t(f - cb.n_win) | 0x80000000u, zero);
                else ++n_cond;
            }
            f = cb.self_next[f];
        }
    }

    if (!FILL) {
        const unsigned long long n = wave_sum_u64(n_cond);
        if (lane == 0) cb.pair_cnt[i] = uint32_t(n);
        return;
    }
    const U128 sum = wave_sum_u128(acc); // the wave's base sum
    if (lane != 0) return;
    cb.base[i] = make_ulonglong2(sum.lo, sum.hi);
    cb.base_flags[i] = uint8_t(tx);
    cb.pair_fill[i] = min(s_np[wave], cap);
}

// The counts' exclusive prefix = the candidates' segments, in three small launches over coalesced reads: every workgroup's sum of
// kCbResolve counts, one workgroup's prefix over those sums (with the total for the host), every workgroup's own prefix on top of its base.
RM_D unsigned long long cb_block_scan(unsigned long long *s_sum, int tid, unsigned long long v) // inclusive, over the workgroup
{
    s_sum[tid] = v;
    __syncthreads();
    for (int d = 1; d < kCbResolve; d <<= 1) {
        const unsigned long long up = tid >= d ? s_sum[tid - d] : 0ull;
        __syncthreads();
        s_sum[tid] += up;
        __syncthreads();
    }
    return s_sum[tid];
}

__global__ void __launch_bounds__(kCbResolve) k_ccab_scan_sums(const CcaBatchDev cb)
{
    __shared__ unsigned long long s_wave[kCbResolve / 64];
    const int tid = threadIdx.x, i = blockIdx.x * kCbResolve + tid;
    const unsigned long long w = wave_sum_u64(i < cb.n_cand ? cb.pair_cnt[i] : 0u);
    if ((tid & 63) == 0) s_wave[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        unsigned long long sum = 0ull;
        for (int k = 0; k < kCbResolve / 64; ++k) sum += s_wave[k];
        cb.pair_base[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(kCbResolve) k_ccab_scan_top(const CcaBatchDev cb, int n_blocks)
{
    __shared__ unsigned long long s_sum[kCbResolve];
    const int tid = threadIdx.x;
    unsigned long long carry = 0ull;
    for (int k0 = 0; k0 < n_blocks; k0 += kCbResolve) { // block-uniform
        const int k = k0 + tid;
        const unsigned long long v = k < n_blocks ? cb.pair_base[k] : 0ull;
        const unsigned long long incl = cb_block_scan(s_sum, tid, v);
        if (k < n_blocks) cb.pair_base[k] = carry + incl - v;
        carry += s_sum[kCbResolve - 1];
        __syncthreads(); // (the next round rewrites the sums)
    }
    if (tid == 0) {
        const bool fits = carry < 0xFFFFFFFFull;
        cb.pair_off[cb.n_cand] = fits ? uint32_t(carry) : 0u;
        cb.h_info[0] = fits ? uint32_t(carry) : 0xFFFFFFFFu; // (does not fit: the host refuses the call, nothing reads the segments)
    }
}

__global__ void __launch_bounds__(kCbResolve) k_ccab_scan_offsets(const CcaBatchDev cb)
{
    __shared__ unsigned long long s_sum[kCbResolve];
    const int tid = threadIdx.x, i = blockIdx.x * kCbResolve + tid;
    const unsigned long long v = i < cb.n_cand ? cb.pair_cnt[i] : 0u;
    const unsigned long long incl = cb_block_scan(s_sum, tid, v);
    if (i < cb.n_cand) cb.pair_off[i] = uint32_t(cb.pair_base[blockIdx.x] + incl - v);
}

// ONE workgroup, the ticks in order: what a candidate of tick b needs of ticks 0 .. b-1 is their kept bits
__global__ void __launch_bounds__(kCbResolve) k_ccab_resolve(const CcaBatchDev cb, double noise_lin, double cca_threshold, int32_t *gated,
                                                              double *out_energy, uint8_t *out_flags)
{
    for (int b = 0; b < cb.n_ticks; ++b) { // block-uniform
        const int first = cb.ticks[b].first, n = cb.ticks[b].n;
        for (int k = threadIdx.x; k < n; k += kCbResolve) {
            const int i = first + k;
            const int j = cb.cand[i];
            double energy = __builtin_nan("");
            uint32_t flags = 0u;
            if (j >= 0) {
                const ulonglong2 b0 = cb.base[i];
                U128 sum = {b0.x, b0.y};
                flags = cb.base_flags[i];
                uint32_t p = cb.pair_off[i];
                const uint32_t p1 = p + cb.pair_fill[i];
                auto take = [&](const uint32_t slot, const ulonglong2 term, const uint8_t on_air) {
                    if (!on_air) return;
                    if (slot >> 31) {
                        flags |= uint32_t(RM_ED_TRANSMITTING);
                    } else {
                        const U128 q = {term.x, term.y};
                        sum = u128_add(sum, q);
                    }
                };
                for (; p + 4u <= p1; p += 4u) { // four pairs in flight: the kept bit is the only dependent load
                    const uint32_t s0 = cb.pair_slot[p], s1 = cb.pair_slot[p + 1], s2 = cb.pair_slot[p + 2], s3 = cb.pair_slot[p + 3];
                    const ulonglong2 t0 = cb.pair_term[p], t1 = cb.pair_term[p + 1], t2 = cb.pair_term[p + 2], t3 = cb.pair_term[p + 3];
                    const uint8_t k0 = cb.kept[s0 & 0x7FFFFFFFu], k1 = cb.kept[s1 & 0x7FFFFFFFu], k2 = cb.kept[s2 & 0x7FFFFFFFu],
                                  k3 = cb.kept[s3 & 0x7FFFFFFFu];
                    take(s0, t0, k0);
                    take(s1, t1, k1);
                    take(s2, t2, k2);
                    take(s3, t3, k3);
                }
                for (; p < p1; ++p) {
                    const uint32_t s0 = cb.pair_slot[p];
                    take(s0, cb.pair_term[p], cb.kept[s0 & 0x7FFFFFFFu]);
                }
                energy = 10.0 * det_log10(q80_to_double(sum) + noise_lin);
                if (energy >= cca_threshold) flags |= uint32_t(RM_ED_BUSY); // (a NaN threshold never sets it)
            }
            const bool keep = j >= 0 && flags == 0u;
            cb.kept[i] = keep ? 1 : 0;
            gated[i] = keep ? j : -1;
            if (out_energy) out_energy[i] = energy;
            if (out_flags) out_flags[i] = uint8_t(flags);
        }
        __syncthreads(); // (the tick's kept bits, for every later tick)
    }
}

// the descriptors and the index's counters; the counts' scan: the CSMA-CA gated batch (rm_csma.hip) takes both as they are
hipError_t launch_ccab_begin(hipStream_t s, const CcaBatchDev &cb, const CcaTick *h_ticks, CcaTick *d_ticks, bool grid)
{
    const int cnt_len = grid ? 2 + kEdCells : 2;
    RM_KLAUNCH(k_ccab_begin, dim3(cdiv(max(cb.n_ticks, cnt_len), 256)), dim3(256), 0, s, h_ticks, cb.n_ticks, d_ticks, cb.cnt, cnt_len);
    return hipGetLastError();
}

hipError_t launch_ccab_scan(hipStream_t s, const CcaBatchDev &cb)
{
    const int n_blocks = cdiv(cb.n_cand, kCbResolve);
    RM_KLAUNCH(k_ccab_scan_sums, dim3(n_blocks), dim3(kCbResolve), 0, s, cb);
    RM_KLAUNCH(k_ccab_scan_top, dim3(1), dim3(kCbResolve), 0, s, cb, n_blocks);
    RM_KLAUNCH(k_ccab_scan_offsets, dim3(n_blocks), dim3(kCbResolve), 0, s, cb);
    return hipGetLastError();
}

hipError_t launch_ccab_count(hipStream_t s, const NodesDev &nd, const ModelDev &m, const CcaBatchDev &cb, const CcaTick *h_ticks, CcaTick *d_ticks, bool grid)
{
    (void)launch_ccab_begin(s, cb, h_ticks, d_ticks, grid);
    const int n_frames = cb.n_win + cb.n_cand;
    if (grid) {
        RM_KLAUNCH((k_ccab_index<true>), dim3(cdiv(n_frames, 256)), dim3(256), 0, s, nd, m, cb);
        RM_KLAUNCH((k_ccab_pairs<true, false>), dim3(cdiv(cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cb);
    } else {
        RM_KLAUNCH((k_ccab_index<false>), dim3(cdiv(n_frames, 256)), dim3(256), 0, s, nd, m, cb);
        RM_KLAUNCH((k_ccab_pairs<false, false>), dim3(cdiv(cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cb);
    }
    return launch_ccab_scan(s, cb);
}

hipError_t launch_ccab_resolve(hipStream_t s, const NodesDev &nd, const ModelDev &m, const CcaBatchDev &cb, bool grid, double cca_threshold,
                               int32_t *gated, double *out_energy, uint8_t *out_flags)
{
    if (grid) RM_KLAUNCH((k_ccab_pairs<true, true>), dim3(cdiv(cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cb);
    else RM_KLAUNCH((k_ccab_pairs<false, true>), dim3(cdiv(cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cb);
    RM_KLAUNCH(k_ccab_resolve, dim3(1), dim3(kCbResolve), 0, s, cb, m.ld_noise_lin, cca_threshold, gated, out_energy, out_flags);
    return hipGetLastError();
}

} // namespace rm
