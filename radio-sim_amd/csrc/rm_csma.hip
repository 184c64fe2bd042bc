// rm_csma.hip -- the gate of a CSMA-CA gated BATCH (rm_batch_run_sources_csma*, _carry*)
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math)
//
// A candidate that finds the channel busy draws a backoff and senses again in a later tick of the batch.  The draw is a hash of the
// packet and the attempt number, so the host knows the tick of every attempt of every packet before the batch starts
// (rm_csma_schedule): every attempt is a SLOT of its tick's expanded list, and the gated batch's architecture (rm_ccabatch.hip) holds
// -- all fp64 once for the whole batch, one workgroup walks the ticks with integer sums.  What is new:
//   k_csma_index     a slot's node comes from its ORIGIN's list entry; its record is built with its own tick's start / air.  Then the
//                    gated batch's index entry (cb_index_frame), with never-live frames on the nodes' chains too.
//   k_csma_pairs     one WAVE per slot, the gated batch's walk (cb_walk).  On the node's chain: a frame of the slot's own packet is
//                    skipped (had it been kept, this attempt would not be made); a frame of an earlier tick is the bit-31 pair; a slot
//                    of the SAME tick at a lower position is a SIBLING pair (bit 30) -- counted in the counting pass too.
//   k_csma_resolve   ONE workgroup, ticks in order, a thread per slot, two phases per tick.  Phase 1: a slot whose packet is still
//                    trying sums its pairs -> flags and a tentative bit.  Phase 2: a slot with sibling pairs loses if a lower sibling
//                    is tentative (one frame per radio per tick: the first in list order wins); kept bit, gated entry, the packet's
//                    state and outputs.  Tentative bits are read and kept bits written in separate arrays.
// The descriptors' copy and the counts' scan are the gated batch's own kernels (launch_ccab_begin, launch_ccab_scan).
// A CARRIED packet (E9) is packet n_pkt + c of the same arrays: its node comes from its carry record, its outputs go to the carried
// table, the first slot of its chain in this batch is marked (kCsFirst) as an own packet's attempt 0 is; one without a slot gets its
// entry before tick 0.
//   k_csma_collect   the carry-out: a stable compaction of the RM_CSMA_PENDING entries, carried table first -- a count per workgroup
//                    (wave ballots), one workgroup's prefix over the counts, then every pending entry's record at its rank.
#include "rm_device.hpp"

namespace rm {

constexpr int kCsResolve = 1024;       // threads of the one workgroup that resolves
constexpr uint8_t kCsTrying = 0xFF;    // CsmaDev::state: attempts so far were made and deferred, another one is scheduled
constexpr uint8_t kCsMade = 0x40;      // CsmaDev::slot_flags: the slot's attempt was made
constexpr int kCsCollect = 256;        // threads of a workgroup of the collect passes: an entry each
constexpr int kCsScan = 1024;          // threads of the one workgroup that scans their counts

template <bool GRID>
__global__ void __launch_bounds__(256) k_csma_index(const NodesDev nd, const ModelDev m, const CsmaDev cs)
{
    const CcaBatchDev &cb = cs.cb;
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
        int lo = 0, hi = cb.n_ticks - 1; // the last tick whose first slot is <= s (empty ticks before it share its offset)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cb.ticks[mid].first <= s) lo = mid;
            else hi = mid - 1;
        }
        tk = lo;
        const int o = cs.origin[s];
        int j;
        if (o >= cs.n_pkt) { // a carried packet: (the host has checked its node)
            j = cs.carry[o - cs.n_pkt].node;
        } else {
            lo = 0, hi = cb.n_ticks - 1; // the origin tick: the last one whose first packet is <= o
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (cs.own_first[mid] <= o) lo = mid;
                else hi = mid - 1;
            }
            j = cb.ticks[lo].src[o - cs.own_first[lo]];
        }
        r = make_tx_record(nd, j, cb.ticks[tk].start_us, cb.ticks[tk].air_us); // (an entry outside 0 .. n-1: a padding record)
        cb.scr[s] = r;
        cb.cand[s] = r.src;
        cb.fr_tick[f] = tk;
        if (r.src < 0) return;
    }
    cb_index_frame<GRID, true>(nd, m, cb, f, r, tk);
}

template <bool GRID, bool FILL>
__global__ void __launch_bounds__(256) k_csma_pairs(const NodesDev nd, const ModelDev m, const CsmaDev cs)
{
    __shared__ uint32_t s_tbl[kShadowBins];
    __shared__ int s_off[kWavesPerBlock][65];
    __shared__ int s_cell[kWavesPerBlock][64];
    __shared__ int64_t s_start[kMaxBatch], s_air[kMaxBatch]; // the ticks' frames: one start and one air time per tick
    __shared__ uint32_t s_np[kWavesPerBlock];                // pairs the wave has appended

    const CcaBatchDev &cb = cs.cb;
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
    const int o = uniform_i(cs.origin[i]);
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
    // (a frame of the slot's own packet is a frame of its own node: ed_candidate leaves it out)
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

    // the node's own frames (its chain), on any channel, whatever their reach: a window frame that spans the sample says
    // RM_ED_TRANSMITTING now; a frame of another packet in an earlier tick says it if it was kept; a slot of another packet in this
    // very tick, earlier in the list, wins over this one if it finds the channel clear
    if (lane == 0) {
        const unsigned long long head = cb.self_slot[j];
        int f = (uint32_t(head >> 32) == cb.stamp) ? int(uint32_t(head)) : -1;
        const U128 zero = {0ull, 0ull};
        while (f >= 0) {
            const int tk = cb.fr_tick[f];
            if (tk < 0) {
                if (cb_live(t, cb.win[f].start_us, cb.win[f].air_us)) tx = uint32_t(RM_ED_TRANSMITTING);
            } else if (cs.origin[f - cb.n_win] != o) {
                const uint32_t slot = uint32_t(f - cb.n_win);
                uint32_t kind = 0u;
                if (tk < b && cb_live(t, s_start[tk], s_air[tk])) kind = kCsOwn;
                else if (tk == b && int(slot) < i) kind = kCsSibling;
                if (kind != 0u) {
                    if (FILL) append(slot | kind, zero);
                    else ++n_cond;
                }
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

// a carried packet whose next attempt is behind the batch has no slot: still pending, nothing sensed
RM_D void cs_slotless(const CsmaDev &cs, int c, int n_ticks)
{
    const rm_csma_carry r = cs.carry[c];
    if (r.tick < n_ticks) return;
    cs.state[cs.n_pkt + c] = uint8_t(RM_CSMA_PENDING);
    if (cs.carried.status) cs.carried.status[c] = uint8_t(RM_CSMA_PENDING);
    if (cs.carried.attempts) cs.carried.attempts[c] = uint8_t(r.attempt);
    if (cs.carried.tick) cs.carried.tick[c] = r.tick;
    if (cs.carried.pkt) cs.carried.pkt[c] = -1;
    if (cs.carried.flags) cs.carried.flags[c] = 0;
    if (cs.carried.energy_dbm) cs.carried.energy_dbm[c] = __builtin_nan("");
}

__global__ void __launch_bounds__(256) k_csma_slotless(const CsmaDev cs, int n_ticks)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < cs.n_carry) cs_slotless(cs, c, n_ticks);
}

// ONE workgroup, the ticks in order: what a slot of tick T needs of ticks 0 .. T-1 is their kept bits and its packet's state
__global__ void __launch_bounds__(kCsResolve) k_csma_resolve(const CsmaDev cs, double noise_lin, double cca_threshold, int32_t *gated)
{
    const CcaBatchDev &cb = cs.cb;
    for (int c = threadIdx.x; c < cs.n_carry; c += kCsResolve) cs_slotless(cs, c, cb.n_ticks); // (entries no slot writes)
    for (int T = 0; T < cb.n_ticks; ++T) { // block-uniform
        const int first = cb.ticks[T].first, n = cb.ticks[T].n;
        // phase 1: every made slot's flags, before the first-wins rule
        for (int k = threadIdx.x; k < n; k += kCsResolve) {
            const int i = first + k;
            const int j = cb.cand[i];
            const int o = cs.origin[i];
            const bool made = j >= 0 && ((cs.attempt[i] & kCsFirst) || cs.state[o] == kCsTrying);
            uint32_t flags = 0u, mark = 0u;
            if (made) {
                const ulonglong2 b0 = cb.base[i];
                U128 sum = {b0.x, b0.y};
                flags = cb.base_flags[i];
                mark = kCsMade;
                uint32_t p = cb.pair_off[i];
                const uint32_t p1 = p + cb.pair_fill[i];
                auto take = [&](const uint32_t slot, const ulonglong2 term, const uint8_t on_air) {
                    if (slot & kCsSibling) {
                        mark |= kCsHasSibling;
                    } else if (on_air) {
                        if (slot & kCsOwn) {
                            flags |= uint32_t(RM_ED_TRANSMITTING);
                        } else {
                            const U128 q = {term.x, term.y};
                            sum = u128_add(sum, q);
                        }
                    }
                };
                for (; p + 4u <= p1; p += 4u) { // four pairs in flight: the kept bit is the only dependent load
                    const uint32_t s0 = cb.pair_slot[p], s1 = cb.pair_slot[p + 1], s2 = cb.pair_slot[p + 2], s3 = cb.pair_slot[p + 3];
                    const ulonglong2 t0 = cb.pair_term[p], t1 = cb.pair_term[p + 1], t2 = cb.pair_term[p + 2], t3 = cb.pair_term[p + 3];
                    const uint8_t k0 = cb.kept[s0 & kCsSlot], k1 = cb.kept[s1 & kCsSlot], k2 = cb.kept[s2 & kCsSlot], k3 = cb.kept[s3 & kCsSlot];
                    take(s0, t0, k0);
                    take(s1, t1, k1);
                    take(s2, t2, k2);
                    take(s3, t3, k3);
                }
                for (; p < p1; ++p) {
                    const uint32_t s0 = cb.pair_slot[p];
                    take(s0, cb.pair_term[p], cb.kept[s0 & kCsSlot]);
                }
                const double energy = 10.0 * det_log10(q80_to_double(sum) + noise_lin);
                if (energy >= cca_threshold) flags |= uint32_t(RM_ED_BUSY); // (a NaN threshold never sets it)
                double *const o_energy = o >= cs.n_pkt ? cs.carried.energy_dbm : cs.out.energy_dbm;
                if (o_energy) o_energy[o >= cs.n_pkt ? o - cs.n_pkt : o] = energy; // (a chain's attempts are in different ticks: one writer)
            }
            cs.tentative[i] = (made && flags == 0u) ? 1 : 0;
            cs.slot_flags[i] = uint8_t(flags | mark);
        }
        __syncthreads(); // (the tick's tentative bits)
        // phase 2: one frame per radio per tick, then the packets' states
        for (int k = threadIdx.x; k < n; k += kCsResolve) {
            const int i = first + k;
            const int j = cb.cand[i];
            const int o = cs.origin[i];
            const int a = cs.attempt[i] & ~kCsFirst; // (a carried packet's attempts count on from those made before this batch)
            const bool chain_first = cs.attempt[i] & kCsFirst;
            const uint32_t sf = cs.slot_flags[i];
            uint32_t flags = sf & uint32_t(RM_ED_TRANSMITTING | RM_ED_BUSY);
            bool keep = cs.tentative[i] != 0;
            if (keep && (sf & kCsHasSibling)) {
                const uint32_t p0 = cb.pair_off[i], p1 = p0 + cb.pair_fill[i];
                for (uint32_t p = p0; p < p1; ++p) {
                    const uint32_t s0 = cb.pair_slot[p];
                    if ((s0 & kCsSibling) && cs.tentative[s0 & kCsSlot]) keep = false;
                }
                if (!keep) flags |= uint32_t(RM_ED_TRANSMITTING); // (its radio starts a frame in this tick)
            }
            cb.kept[i] = keep ? 1 : 0;
            gated[i] = keep ? j : -1;
            if (sf & kCsMade) {
                const int nt = cs.next_tick[i];
                const uint8_t st = keep ? uint8_t(RM_CSMA_SENT) : nt < 0 ? uint8_t(RM_CSMA_FAILED) : nt >= cb.n_ticks ? uint8_t(RM_CSMA_PENDING) : kCsTrying;
                cs.state[o] = st;
                // the table the packet belongs to
                const bool car = o >= cs.n_pkt;
                const int e = car ? o - cs.n_pkt : o;
                uint8_t *const o_status = car ? cs.carried.status : cs.out.status;
                uint8_t *const o_attempts = car ? cs.carried.attempts : cs.out.attempts;
                uint8_t *const o_flags = car ? cs.carried.flags : cs.out.flags;
                int32_t *const o_tick = car ? cs.carried.tick : cs.out.tick;
                int32_t *const o_pkt = car ? cs.carried.pkt : cs.out.pkt;
                if (o_attempts) o_attempts[e] = uint8_t(a + 1);
                if (o_flags) o_flags[e] = uint8_t(flags);
                if (st != kCsTrying) {
                    if (o_status) o_status[e] = st;
                    if (o_tick) o_tick[e] = keep ? T : st == RM_CSMA_PENDING ? nt : -1;
                    if (o_pkt) o_pkt[e] = keep ? k : -1;
                }
            } else if (chain_first) { // a padding entry: a packet that never attempts (an own one: a carried packet's node is a node)
                cs.state[o] = uint8_t(RM_CSMA_NONE);
                if (cs.out.status) cs.out.status[o] = uint8_t(RM_CSMA_NONE);
                if (cs.out.attempts) cs.out.attempts[o] = 0;
                if (cs.out.tick) cs.out.tick[o] = -1;
                if (cs.out.pkt) cs.out.pkt[o] = -1;
                if (cs.out.flags) cs.out.flags[o] = 0;
                if (cs.out.energy_dbm) cs.out.energy_dbm[o] = __builtin_nan("");
            }
        }
        __syncthreads(); // (the tick's kept bits and states, for every later tick)
    }
}

// ---- the carry-out (E9) ---------------------------------------------------------------------------------------------------------
// entry e of the two tables as one: the carried packets, then the own ones
RM_D bool cc_pending(const CsmaCollectDev &cc, int e)
{
    if (e >= cc.n_carry + cc.n_pkt) return false;
    return (e < cc.n_carry ? cc.status[0][e] : cc.status[1][e - cc.n_carry]) == uint8_t(RM_CSMA_PENDING);
}

// FILL = false: the workgroup's pending entries; FILL = true (after the scan): every pending entry's record at its rank
template <bool FILL>
__global__ void __launch_bounds__(kCsCollect) k_csma_collect(const CsmaCollectDev cc)
{
    __shared__ uint32_t s_wave[kCsCollect / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const int e = blockIdx.x * kCsCollect + tid;
    const bool pending = cc_pending(cc, e);
    const unsigned long long mask = __ballot(pending);
    if (lane == 0) s_wave[wave] = uint32_t(__popcll(mask));
    __syncthreads();
    if (!FILL) {
        if (tid == 0) {
            uint32_t sum = 0u;
            for (int w = 0; w < kCsCollect / 64; ++w) sum += s_wave[w];
            cc.block_cnt[blockIdx.x] = sum;
        }
        return;
    }
    if (!pending) return;
    unsigned long long rank = cc.block_cnt[blockIdx.x];
    for (int w = 0; w < wave; ++w) rank += s_wave[w];
    rank += uint32_t(__popcll(mask & ((1ull << lane) - 1ull)));
    if (rank >= (unsigned long long)cc.cap) return; // (the host reports RM_ERR_CAPACITY with the count)
    rm_csma_carry r;
    if (e < cc.n_carry) {
        r = cc.carry[e];
        r.tick = cc.tick[0][e] - cc.n_ticks;
        r.attempt = cc.attempts[0][e];
    } else {
        const int o = e - cc.n_carry;
        int lo = 0, hi = cc.n_ticks - 1; // the origin tick: the last one whose first packet is <= o
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cc.own_first[mid] <= o) lo = mid;
            else hi = mid - 1;
        }
        r.origin_cca_time_us = cc.cca_us[lo];
        r.origin_slot = o - cc.own_first[lo];
        r.node = cc.src[lo][r.origin_slot];
        r.tick = cc.tick[1][o] - cc.n_ticks;
        r.attempt = cc.attempts[1][o];
    }
    cc.h_out[rank] = r;
}

// one workgroup: the workgroups' counts -> the entries before each of them; the total for the host
__global__ void __launch_bounds__(kCsScan) k_csma_collect_scan(const CsmaCollectDev cc, int n_blocks)
{
    __shared__ unsigned long long s_sum[kCsScan];
    const int tid = threadIdx.x;
    unsigned long long before = 0ull;
    for (int k0 = 0; k0 < n_blocks; k0 += kCsScan) { // block-uniform
        const int k = k0 + tid;
        const unsigned long long own = k < n_blocks ? cc.block_cnt[k] : 0ull;
        s_sum[tid] = own;
        __syncthreads();
        for (int d = 1; d < kCsScan; d <<= 1) {
            const unsigned long long add = tid >= d ? s_sum[tid - d] : 0ull;
            __syncthreads();
            s_sum[tid] += add;
            __syncthreads();
        }
        // (a carry-out of 2^32 entries or more does not exist: at most 2^27 packets)
        if (k < n_blocks) cc.block_cnt[k] = uint32_t(before + s_sum[tid] - own);
        before += s_sum[kCsScan - 1];
        __syncthreads();
    }
    if (tid == 0) *cc.h_count = before;
}

hipError_t launch_csma_collect(hipStream_t s, const CsmaCollectDev &cc)
{
    const int n_blocks = cdiv(cc.n_carry + cc.n_pkt, kCsCollect);
    RM_KLAUNCH((k_csma_collect<false>), dim3(n_blocks), dim3(kCsCollect), 0, s, cc);
    RM_KLAUNCH(k_csma_collect_scan, dim3(1), dim3(kCsScan), 0, s, cc, n_blocks);
    RM_KLAUNCH((k_csma_collect<true>), dim3(n_blocks), dim3(kCsCollect), 0, s, cc);
    return hipGetLastError();
}

hipError_t launch_csma_slotless(hipStream_t s, const CsmaDev &cs)
{
    RM_KLAUNCH(k_csma_slotless, dim3(cdiv(cs.n_carry, 256)), dim3(256), 0, s, cs, cs.cb.n_ticks);
    return hipGetLastError();
}

hipError_t launch_csma_count(hipStream_t s, const NodesDev &nd, const ModelDev &m, const CsmaDev &cs, const CcaTick *h_ticks, CcaTick *d_ticks, bool grid)
{
    (void)launch_ccab_begin(s, cs.cb, h_ticks, d_ticks, grid);
    const int n_frames = cs.cb.n_win + cs.cb.n_cand;
    if (grid) {
        RM_KLAUNCH((k_csma_index<true>), dim3(cdiv(n_frames, 256)), dim3(256), 0, s, nd, m, cs);
        RM_KLAUNCH((k_csma_pairs<true, false>), dim3(cdiv(cs.cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cs);
    } else {
        RM_KLAUNCH((k_csma_index<false>), dim3(cdiv(n_frames, 256)), dim3(256), 0, s, nd, m, cs);
        RM_KLAUNCH((k_csma_pairs<false, false>), dim3(cdiv(cs.cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cs);
    }
    return launch_ccab_scan(s, cs.cb);
}

hipError_t launch_csma_resolve(hipStream_t s, const NodesDev &nd, const ModelDev &m, const CsmaDev &cs, bool grid, double cca_threshold, int32_t *gated)
{
    if (grid) RM_KLAUNCH((k_csma_pairs<true, true>), dim3(cdiv(cs.cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cs);
    else RM_KLAUNCH((k_csma_pairs<false, true>), dim3(cdiv(cs.cb.n_cand, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, cs);
    RM_KLAUNCH(k_csma_resolve, dim3(1), dim3(kCsResolve), 0, s, cs, m.ld_noise_lin, cca_threshold, gated);
    return hipGetLastError();
}

} // namespace rm
