// rm_energy.hip -- channel energy query (CCA / ED): how much power does a node see on a channel right now?
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math)
//
// The read side of the SINR extension's state (not reference behaviour -- the reference answers
// with the latched RSSI of a frame being received, or a constant).  The frames on the air are the context's on-air window
// (rm_context::d_air[air_head, air_tail)); a query at time t sums, for every queried node j on channel c, the linear
// power of every frame of the window that is live at t, on channel c, not j's own, and reaches the interference floor at
// j -- the exact integer Q80 sum of E3 -- and answers 10 log10(sum + noise).  Two launches, nothing kept between queries:
//   k_energy_index   one thread per record of the window: frames live at t get their pre-filter record at the
//                    interference-floor level (tx_prefilter_at: fp32 position, squared cut-off with the filter's margins,
//                    clip-widened when the medium shadows) and go into a kEdG x kEdG grid over the fp32 frame (up to kEdK per
//                    cell) or, without a bound or a place, into the EVERY list; the source node of a live frame gets the
//                    query's stamp (RM_ED_TRANSMITTING).  Below kEdSmallWindow records there is no grid: every frame goes
//                    into the EVERY list.
//   k_energy_sum     one lane per queried node (in the receiver table's spatial order when all nodes are asked for, so
//                    that a wave walks the same cells).  A lane walks the cells within the largest cut-off radius of its
//                    node; the EVERY list is staged in LDS, 256 records at a time, and swept by every lane.  Candidates
//                    pass the sweep's conservative tests (channel, fp32 distance against the cut-off, the shadowed
//                    medium's link-hash table); the survivors of a wave are gathered in LDS and evaluated with full lanes
//                    -- logdist_rssi in fp64, det_pow10, Q80 -- and added to their node's sum in LDS (integer adds: the
//                    order does not matter).
//   k_cca_gate       the gate of a carrier-sense gated tick (E6; further down): the same index, one WAVE per candidate.
// The conservative tests only ever drop work: a frame that counts (E5) always reaches the exact evaluation, whatever the
// grid, the lists' order or the path.
#include "rm_device.hpp"

namespace rm {

constexpr int kEdPairs = 256; // surviving (node, frame) pairs a wave gathers between two exact phases
constexpr int kEdChunk = 256; // records of the EVERY list staged in LDS together
static_assert(kEdChunk == kBlock && kShadowBins == kBlock, "one record / one table entry per thread");

RM_D void ed_add_u128(unsigned long long *acc /*[2]: lo, hi*/, const U128 v)
{
    if ((v.lo | v.hi) == 0ull) return;
    const unsigned long long old = atomicAdd(&acc[0], (unsigned long long)v.lo);
    const unsigned long long carry = (old + v.lo < old) ? 1ull : 0ull; // (the low words' running sum is exact mod 2^64: so is the carry count)
    if (v.hi + carry) atomicAdd(&acc[1], (unsigned long long)(v.hi + carry));
}

template <bool GRID>
__global__ void __launch_bounds__(256) k_energy_index(const ModelDev m, const rm_tx_record *win, int n_win, int n_nodes, int64_t t, const EnergyDev ed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_win) return;
    const rm_tx_record r = win[i];
    // live at t: start <= t < start + air (the end of a span is exclusive)
    if (r.src < 0 || t < r.start_us || t - r.start_us >= r.air_us) return;
    if (r.src < n_nodes) ed.tx_mark[r.src] = ed.stamp;
    float4 f;
    double thr64;
    tx_prefilter_at(m, m.ld_ifloor, r, f, thr64);
    if (!(f.w >= 0.f)) return; // reaches the floor nowhere
    float inv = 0.f;           // squared fp32 distance -> bin of the link-hash table (0: the table says nothing about this frame)
    if (m.shadow_tbl != nullptr && f.w > 0.f && f.w < __builtin_inff()) { // (the sweep's second-level filter, rm_tick.hip)
        const float cut = __builtin_sqrtf(f.w);
        if (1.01f * (2.0f * float(m.f32_slack)) / (0.15f * cut) + 1e-5f <= float(kShadowPad)) inv = float(kShadowBins) / f.w;
    }
    const int4 meta = make_int4(r.channel, i, r.src, __float_as_int(inv));
    if (GRID && f.w < __builtin_inff()) {
        const int cell = sg_cell1(f.y, ed.half, ed.inv) * kEdG + sg_cell1(f.x, ed.half, ed.inv);
        atomicMax(&ed.cnt[1], __float_as_uint(sqrt_up(f.w))); // (radii are >= 0: their bits order like they do)
        const uint32_t k = atomicAdd(&ed.cnt[2 + cell], 1u);
        if (k < uint32_t(kEdK)) {
            ed.bucket_f[cell * kEdK + int(k)] = f;
            ed.bucket_m[cell * kEdK + int(k)] = meta;
            return;
        }
    }
    const uint32_t e = atomicAdd(&ed.cnt[0], 1u); // no bound, outside the frame, the cell is full, or no grid at all
    ed.every_f[e] = f;
    ed.every_m[e] = meta;
}

template <bool GRID>
__global__ void __launch_bounds__(256) k_energy_sum(const NodesDev nd, const ModelDev m, const rm_tx_record *win, const EnergyDev ed,
                                                     const int32_t *nodes, int n, int channel, double cca_threshold, double *out_energy,
                                                     uint8_t *out_flags)
{
    __shared__ double s_x[kBlock], s_y[kBlock], s_z[kBlock]; // the lanes' nodes: position ...
    __shared__ int s_j[kBlock];                              // ... node index
    __shared__ unsigned long long s_acc[kBlock * 2];         // Q80 sum per node
    __shared__ uint32_t s_pf[kWavesPerBlock * kEdPairs];     // surviving pairs of a wave: frame ...
    __shared__ uint8_t s_pl[kWavesPerBlock * kEdPairs];      // ... and lane
    __shared__ float4 s_ef[kEdChunk];                        // a chunk of the EVERY list
    __shared__ int4 s_em[kEdChunk];
    __shared__ uint32_t s_tbl[kShadowBins];

    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const int k = blockIdx.x * blockDim.x + tid;
    const bool shadow = m.shadow_tbl != nullptr;
    s_tbl[tid] = shadow ? m.shadow_tbl[tid] : 0xFFFFFFFFu;
    // which node, and where its result goes: all nodes in the receiver table's order, written by node index; a list by its entries
    // (no list and fewer than all: nodes 0 .. n-1)
    const bool all = nodes == nullptr && n == nd.n_rx;
    int j = -1, o = k;
    if (k < n) {
        if (nodes) j = nodes[k];
        else if (all) j = o = nd.orig[k];
        else j = k;
    }
    const bool valid = j >= 0 && j < nd.n;
    double x = 0.0, y = 0.0, z = 0.0;
    int ch = 0;
    if (valid) {
        if (all) { // (engine order: coalesced)
            x = nd.x[k], y = nd.y[k], z = nd.z[k];
            ch = nd.channel[k];
        } else {
            const SrcRecord sr = nd.srec[j];
            x = sr.x, y = sr.y, z = sr.z;
            ch = sr.channel;
        }
    }
    if (channel != RM_CHANNEL_OWN) ch = channel;
    const double rx_ = x - m.org_x, ry_ = y - m.org_y, rz_ = z - m.org_z;
    const float px = float(rx_), py = float(ry_), pz = float(rz_);
    // a node outside the frame the fp32 slack was computed for takes every co-channel frame as a candidate
    const bool wide = !(fabs(rx_) <= m.coord_bound && fabs(ry_) <= m.coord_bound && fabs(rz_) <= m.coord_bound);
    const EdNode nv{valid, wide, shadow, ch, j, px, py, pz};
    s_x[tid] = x;
    s_y[tid] = y;
    s_z[tid] = z;
    s_j[tid] = j;
    s_acc[tid * 2] = s_acc[tid * 2 + 1] = 0ull;
    __syncthreads(); // (the table)

    // ---- a wave's surviving pairs, evaluated with full lanes whenever the next ballot might not fit
    int np = 0; // wave-uniform
    auto exact = [&]() {
        for (int pp = lane; pp < np; pp += 64) {
            const int l = wave * 64 + int(s_pl[wave * kEdPairs + pp]);
            const rm_tx_record w = win[s_pf[wave * kEdPairs + pp]];
            const int dst = s_j[l];
            const double rssi = logdist_rssi(m, w, s_x[l], s_y[l], s_z[l], dst);
            if (rssi >= m.ld_ifloor) ed_add_u128(&s_acc[l * 2], q80_from_double(det_pow10(rssi / 10.0)));
        }
        np = 0;
    };
    auto append = [&](const bool hit, const int frame) {
        const uint64_t hm = ballot64(hit);
        const int cnt = int(__popcll(hm));
        if (cnt == 0) return;
        if (np + cnt > kEdPairs) exact(); // wave-uniform: room first
        if (hit) {
            const int at = wave * kEdPairs + np + int(lane_prefix(hm));
            s_pf[at] = uint32_t(frame);
            s_pl[at] = uint8_t(lane);
        }
        np += cnt;
    };
    auto candidate = [&](const float4 &f, const int4 &fm) -> bool { return ed_candidate(m, s_tbl, nv, f, fm); };

    if (GRID) {
        // the cells that can hold a frame within reach: |dx| <= (largest radius), and positions map to cells monotonically
        const float rmax = __uint_as_float(ed.cnt[1]);
        const float reach = rmax * (1.0f + 2e-5f) + 1e-3f / ed.inv;
        int cx0 = 0, cy0 = 0, cx1 = kEdG - 1, cy1 = kEdG - 1;
        if (!wide) {
            cx0 = sg_cell1(px - reach, ed.half, ed.inv);
            cx1 = sg_cell1(px + reach, ed.half, ed.inv);
            cy0 = sg_cell1(py - reach, ed.half, ed.inv);
            cy1 = sg_cell1(py + reach, ed.half, ed.inv);
        }
        int cx = cx0, cy = cy0, e = 0;
        bool done = !valid;
        int cell = cy * kEdG + cx;
        int ccnt = done ? 0 : int(min(ed.cnt[2 + cell], uint32_t(kEdK)));
        for (;;) {
            bool have = false;
            float4 f = make_float4(0.f, 0.f, 0.f, -1.f);
            int4 fm = make_int4(0, 0, 0, 0);
            while (!done && !have) {
                if (e < ccnt) {
                    f = ed.bucket_f[cell * kEdK + e];
                    fm = ed.bucket_m[cell * kEdK + e];
                    ++e;
                    have = true;
                } else {
                    e = 0;
                    if (++cx > cx1) {
                        cx = cx0;
                        if (++cy > cy1) done = true;
                    }
                    if (!done) {
                        cell = cy * kEdG + cx;
                        ccnt = int(min(ed.cnt[2 + cell], uint32_t(kEdK)));
                    }
                }
            }
            if (ballot64(have) == 0ull) break;
            append(have && candidate(f, fm), fm.y);
        }
    }
    // the EVERY list: staged in LDS, swept by every lane
    const int n_every = uniform_i(int(ed.cnt[0]));
    for (int e0 = 0; e0 < n_every; e0 += kEdChunk) { // block-uniform
        const int ne = min(kEdChunk, n_every - e0);
        __syncthreads(); // (the chunk before is done with)
        if (tid < ne) {
            s_ef[tid] = ed.every_f[e0 + tid];
            s_em[tid] = ed.every_m[e0 + tid];
        }
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const int4 fm = s_em[e];
            append(candidate(s_ef[e], fm), fm.y);
        }
    }
    exact();

    if (k >= n) return;
    double energy = __builtin_nan("");
    uint32_t flags = 0u;
    if (valid) {
        U128 acc;
        acc.lo = s_acc[tid * 2];
        acc.hi = s_acc[tid * 2 + 1];
        energy = 10.0 * det_log10(q80_to_double(acc) + m.ld_noise_lin);
        if (ed.tx_mark[j] == ed.stamp) flags |= uint32_t(RM_ED_TRANSMITTING);
        if (energy >= cca_threshold) flags |= uint32_t(RM_ED_BUSY); // (a NaN threshold never sets it)
    }
    out_energy[o] = energy;
    if (out_flags) out_flags[o] = uint8_t(flags);
}

hipError_t launch_energy(hipStream_t s, const NodesDev &nd, const ModelDev &m, const rm_tx_record *win, int n_win, int64_t t, const EnergyDev &ed,
                         bool grid, const int32_t *nodes, int n, int channel, double cca_threshold, double *out_energy, uint8_t *out_flags)
{
    if (n_win > 0) {
        if (grid) RM_KLAUNCH((k_energy_index<true>), dim3(cdiv(n_win, 256)), dim3(256), 0, s, m, win, n_win, nd.n, t, ed);
        else RM_KLAUNCH((k_energy_index<false>), dim3(cdiv(n_win, 256)), dim3(256), 0, s, m, win, n_win, nd.n, t, ed);
    }
    if (n <= 0) return hipGetLastError();
    if (grid) RM_KLAUNCH((k_energy_sum<true>), dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, nd, m, win, ed, nodes, n, channel, cca_threshold, out_energy, out_flags);
    else RM_KLAUNCH((k_energy_sum<false>), dim3(cdiv(n, kBlock)), dim3(kBlock), 0, s, nd, m, win, ed, nodes, n, channel, cca_threshold, out_energy, out_flags);
    return hipGetLastError();
}

// ---- the gate of a carrier-sense gated tick (rm_tick_run_sources_cca*) ----------------------------------
// One WAVE per candidate transmitter.  The query's list form gives every lane a scattered node of its own, and the lane walks its
// cells one dependent memory round trip after the other; here the lanes of a wave share one node: they read the counts of the cells
// in reach together (one lane per cell), a wave prefix turns the counts into one flat range of entries, and the lanes stride over
// that range and then over the EVERY list.  A lane evaluates its survivors where it stands (fp64, Q80) into a 128-bit partial sum
// of its own; the wave adds the partial sums as integers -- 32-bit limbs, each summed in 64 bits across the lanes, carries
// propagated once at the end -- so that the order cannot matter.  Lane 0 forms the energy and the flags and writes the gated
// source: the candidate itself when the channel is clear, -1 (a padding record: make_tx_record) when it defers.
template <bool GRID>
__global__ void __launch_bounds__(256) k_cca_gate(const NodesDev nd, const ModelDev m, const rm_tx_record *win, const EnergyDev ed,
                                                   const int32_t *src, int n, double cca_threshold, int32_t *gated, double *out_energy,
                                                   uint8_t *out_flags)
{
    __shared__ uint32_t s_tbl[kShadowBins];
    __shared__ int s_off[kWavesPerBlock][65]; // a wave's cells of one round: first entry of each in the flat range ...
    __shared__ int s_cell[kWavesPerBlock][64]; // ... and which cell it is

    const int tid = threadIdx.x, lane = tid & 63, wave = wave_index();
    const bool shadow = m.shadow_tbl != nullptr;
    s_tbl[tid] = shadow ? m.shadow_tbl[tid] : 0xFFFFFFFFu;
    __syncthreads(); // (the table; the waves go their own ways from here)
    const int i = blockIdx.x * kWavesPerBlock + wave; // wave-uniform
    if (i >= n) return;
    const int j = uniform_i(src[i]);
    if (!(j >= 0 && j < nd.n)) { // padding stays padding
        if (lane == 0) {
            gated[i] = -1;
            if (out_energy) out_energy[i] = __builtin_nan("");
            if (out_flags) out_flags[i] = 0;
        }
        return;
    }
    const SrcRecord sr = nd.srec[j];
    const double rx_ = sr.x - m.org_x, ry_ = sr.y - m.org_y, rz_ = sr.z - m.org_z;
    const float px = float(rx_), py = float(ry_), pz = float(rz_);
    const bool wide = !(fabs(rx_) <= m.coord_bound && fabs(ry_) <= m.coord_bound && fabs(rz_) <= m.coord_bound);
    const EdNode nv{true, wide, shadow, sr.channel, j, px, py, pz};

    U128 acc = {0ull, 0ull};
    auto look = [&](const float4 &f, const int4 &fm) {
        if (!ed_candidate(m, s_tbl, nv, f, fm)) return;
        const double rssi = logdist_rssi(m, win[fm.y], sr.x, sr.y, sr.z, j);
        if (rssi >= m.ld_ifloor) acc = u128_add(acc, q80_from_double(det_pow10(rssi / 10.0)));
    };

    if (GRID) {
        // the cells that can hold a frame within reach (as the query: |dx| <= largest radius, positions map to cells monotonically)
        const float rmax = __uint_as_float(ed.cnt[1]);
        const float reach = rmax * (1.0f + 2e-5f) + 1e-3f / ed.inv;
        int cx0 = 0, cy0 = 0, cx1 = kEdG - 1, cy1 = kEdG - 1;
        if (!wide) {
            cx0 = sg_cell1(px - reach, ed.half, ed.inv);
            cx1 = sg_cell1(px + reach, ed.half, ed.inv);
            cy0 = sg_cell1(py - reach, ed.half, ed.inv);
            cy1 = sg_cell1(py + reach, ed.half, ed.inv);
        }
        cx0 = uniform_i(cx0), cx1 = uniform_i(cx1), cy0 = uniform_i(cy0), cy1 = uniform_i(cy1);
        const int ncx = cx1 - cx0 + 1, ncells = ncx * (cy1 - cy0 + 1);
        for (int c0 = 0; c0 < ncells; c0 += 64) { // wave-uniform; one round for a node inside the frame with the usual reach
            const int c = c0 + lane;
            int cell = 0, cnt = 0;
            if (c < ncells) {
                cell = (cy0 + c / ncx) * kEdG + cx0 + c % ncx;
                cnt = int(min(ed.cnt[2 + cell], uint32_t(kEdK))); // first round trip: every cell's count at once
            }
            int incl = cnt; // inclusive prefix over the wave
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const int total = uniform_i(__shfl(incl, 63));
            if (total == 0) continue;
            s_off[wave][lane] = incl - cnt;
            s_cell[wave][lane] = cell;
            if (lane == 63) s_off[wave][64] = total;
            __builtin_amdgcn_wave_barrier(); // (LDS traffic of one wave is in order; the compiler must not move it either)
            for (int e = lane; e < total; e += 64) { // second round trip: the entries, whichever cell they are in
                int lo = 0;                              // the last cell whose first entry is <= e (empty cells before it share its offset)
                for (int step = 32; step > 0; step >>= 1)
                    if (s_off[wave][lo + step] <= e) lo += step;
                const int at = s_cell[wave][lo] * kEdK + (e - s_off[wave][lo]);
                look(ed.bucket_f[at], ed.bucket_m[at]);
            }
            __builtin_amdgcn_wave_barrier(); // (the next round rewrites the offsets)
        }
    }
    const int n_every = uniform_i(int(ed.cnt[0]));
    for (int e = lane; e < n_every; e += 64) look(ed.every_f[e], ed.every_m[e]);

    // the wave's sum: four 32-bit limbs, each added across the lanes in 64 bits (64 x 2^32 fits easily), carries once
    const unsigned long long l0 = wave_sum_u64(acc.lo & 0xFFFFFFFFull), l1 = wave_sum_u64(acc.lo >> 32);
    const unsigned long long l2 = wave_sum_u64(acc.hi & 0xFFFFFFFFull), l3 = wave_sum_u64(acc.hi >> 32);
    if (lane != 0) return;
    U128 sum, part;
    sum.lo = l0, sum.hi = l2;
    part.lo = l1 << 32, part.hi = (l1 >> 32) + (l3 << 32); // (mod 2^128, as the query's sums)
    sum = u128_add(sum, part);
    const double energy = 10.0 * det_log10(q80_to_double(sum) + m.ld_noise_lin);
    uint32_t flags = 0u;
    if (ed.tx_mark[j] == ed.stamp) flags |= uint32_t(RM_ED_TRANSMITTING);
    if (energy >= cca_threshold) flags |= uint32_t(RM_ED_BUSY); // (a NaN threshold never sets it)
    gated[i] = flags ? -1 : j;
    if (out_energy) out_energy[i] = energy;
    if (out_flags) out_flags[i] = uint8_t(flags);
}

hipError_t launch_cca_gate(hipStream_t s, const NodesDev &nd, const ModelDev &m, const rm_tx_record *win, int n_win, int64_t t, const EnergyDev &ed,
                           bool grid, const int32_t *src, int n, double cca_threshold, int32_t *gated, double *out_energy, uint8_t *out_flags)
{
    if (n_win > 0) {
        if (grid) RM_KLAUNCH((k_energy_index<true>), dim3(cdiv(n_win, 256)), dim3(256), 0, s, m, win, n_win, nd.n, t, ed);
        else RM_KLAUNCH((k_energy_index<false>), dim3(cdiv(n_win, 256)), dim3(256), 0, s, m, win, n_win, nd.n, t, ed);
    }
    if (n <= 0) return hipGetLastError();
    if (grid) RM_KLAUNCH((k_cca_gate<true>), dim3(cdiv(n, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, win, ed, src, n, cca_threshold, gated, out_energy, out_flags);
    else RM_KLAUNCH((k_cca_gate<false>), dim3(cdiv(n, kWavesPerBlock)), dim3(kBlock), 0, s, nd, m, win, ed, src, n, cca_threshold, gated, out_energy, out_flags);
    return hipGetLastError();
}

} // namespace rm
