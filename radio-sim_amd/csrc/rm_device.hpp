// rm_device.hpp -- device-side building blocks shared by the kernels: wave helpers, pre-filter records, eval_link, fused scans
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
#pragma once

#include "rm_math.hpp"

namespace rm {

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

RM_D float wave_min(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
RM_D float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}
RM_D int wave_max_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

RM_D float round_up_to_float(double v)
{
    float f = float(v);
    if (double(f) < v) f = nextafterf(f, __builtin_inff());
    return f;
}

// Pre-filter record of one frame: position in the fp32 frame + threshold on the squared fp32
// distance (and the fp64 threshold for the fp64 variant).  thr < 0: nobody can be a candidate;
// thr = +inf: every enabled same-channel receiver is one (non-geometric media, or a frame whose
// position lies outside the frame the fp32 slack was computed for).
RM_D void tx_prefilter_at(const ModelDev &m, const double level, const rm_tx_record &tx, float4 &f, double &thr64);
RM_D void tx_prefilter(const ModelDev &m, const rm_tx_record &tx, float4 &f, double &thr64) { tx_prefilter_at(m, m.ld_level, tx, f, thr64); }
// (the same with the level given: the log-distance medium's cut-off at another level than the model's candidate level)
RM_D void tx_prefilter_at(const ModelDev &m, const double level, const rm_tx_record &tx, float4 &f, double &thr64)
{
    const double inf = u2f(0x7FF0000000000000ull);
    double cut; // cut-off distance (metres): no link beyond it can matter
    if (tx.src < 0) {
        cut = -1.0; // padding record
    } else if (m.kind == RM_MODEL_UDGM || m.kind == RM_MODEL_UDGM_CONST) {
        cut = m.geo_cut;
    } else if (m.kind == RM_MODEL_LOGDIST) {
        const double margin = tx.txpower - m.ld_pl0 + m.ld_sigma * m.ld_clip - (level - 1e-6);
        if (!(margin >= 0.0)) {
            cut = -1.0;
        } else if (!(m.ld_exp > 0.0)) {
            cut = inf;
        } else {
            // hardware fp32 exp2 (relative error ~1e-6 at these arguments) with a 1e-4 pad
            cut = m.ld_d0 * double(__builtin_amdgcn_exp2f(float(margin * m.ld_cut_scale))) * (1.0 + 1e-4);
            if (cut < m.ld_d0) cut = m.ld_d0;
        }
    } else {
        cut = inf; // Null / N2N: no geometry
    }
    const double rx_ = tx.x - m.org_x, ry_ = tx.y - m.org_y, rz_ = tx.z - m.org_z;
    const bool geometric = (m.kind == RM_MODEL_UDGM || m.kind == RM_MODEL_UDGM_CONST || m.kind == RM_MODEL_LOGDIST);
    const bool in_frame = fabs(rx_) <= m.coord_bound && fabs(ry_) <= m.coord_bound && fabs(rz_) <= m.coord_bound;
    f.x = f.y = f.z = 0.f;
    if (cut < 0.0) {
        f.w = -1.f;
        thr64 = -1.0;
    } else if (!geometric || !in_frame || cut == inf) {
        f.w = __builtin_inff();
        thr64 = inf;
        if (geometric && in_frame) {
            f.x = float(rx_);
            f.y = float(ry_);
            f.z = float(rz_);
        }
    } else {
        f.x = float(rx_);
        f.y = float(ry_);
        f.z = float(rz_);
        const double eps = 0x1.0p-24;
        const double c = cut + m.f32_slack + 4.0 * eps * cut;
        f.w = round_up_to_float(c * c * (1.0 + 16.0 * eps));
        thr64 = (cut * cut) * (1.0 + 1e-12);
    }
}

// One frame on the air, indexed for the second launch of a tick by scan (rm_airscan.hip; ScanDev):
// where it is in the fp32 frame and how far it can matter at the level of `m` -- the pre-filter's own cut-off, as a radius --,
// its cell of the frame grid, and its place in its source node's chain of frames (half duplex does not ask for reach).
RM_D float sqrt_up(float v) { return nextafterf(__builtin_sqrtf(v), __builtin_inff()); }
RM_D int sg_cell1(float x, float half, float inv) // (monotone in x: a range of positions maps to a range of cells)
{
    const int c = int((x + half) * inv);
    return min(max(c, 0), kSgG - 1);
}
RM_D void scan_index(const ModelDev &m, const TickDev &t, const ScanDev &sd, int n_nodes, int i, const rm_tx_record &r)
{
    float4 f;
    double thr64;
    tx_prefilter(m, r, f, thr64);
    const bool on_air = r.src >= 0 && r.src < n_nodes && r.start_us + r.air_us > t.air.t_begin;
    float rad = -1.f;
    if (on_air && f.w >= 0.f) rad = (f.w < __builtin_inff()) ? sqrt_up(f.w) : __builtin_inff();
    sd.xyzr[i] = make_float4(f.x, f.y, f.z, rad);
    sd.ch[i] = r.channel;
    if (!on_air) return;
    const unsigned long long stamp = (unsigned long long)sd.stamp << 32;
    const unsigned long long old = atomicExch(&sd.self_slot[r.src], stamp | (unsigned long long)uint32_t(i));
    sd.self_next[i] = ((old >> 32) == sd.stamp) ? int(uint32_t(old)) : -1;
    if (rad < 0.f) return;
    bool placed = false;
    if (rad < __builtin_inff()) {
        const int cell = sg_cell1(f.y, sd.half, sd.inv) * kSgG + sg_cell1(f.x, sd.half, sd.inv);
        const uint32_t k = atomicAdd(&sd.cnt[cell], 1u);
        if (k < uint32_t(kSgK)) {
            sd.bucket_xyzr[cell * kSgK + int(k)] = make_float4(f.x, f.y, f.z, rad);
            sd.bucket_ci[cell * kSgK + int(k)] = make_int2(r.channel, i);
            placed = true;
        }
        atomicMax(&sd.cnt[kSgCells + 1 + (i & (kSgMax - 1))], __float_as_uint(rad)); // (radii are >= 0: their bits order like they do)
    }
    if (!placed) sd.every[atomicAdd(&sd.cnt[kSgCells], 1u)] = uint32_t(i); // no bound, or the cell is full: everybody looks at it
}

// engine position of a node in this partition's receiver table, -1 = not a receiver here (another rank's node, padding)
RM_D int engine_pos(const NodesDev &nd, int node)
{
    const uint32_t k = uint32_t(node - nd.rx_first);
    return (k < uint32_t(nd.pos_span)) ? nd.pos_of[k] : -1;
}

// RadioPacket(node, time, data): copies the source radio's txpower / channel (RadioPacket.java:46-52)
RM_D rm_tx_record make_tx_record(const NodesDev &nd, int s, int64_t start_us, int64_t air_us)
{
    rm_tx_record r;
    if (s < 0 || s >= nd.n) { // padding slot
        r.x = r.y = r.z = 0.0;
        r.txpower = 0.0;
        r.txprob = 0.0;
        r.start_us = start_us;
        r.air_us = 0;
        r.src = -1;
        r.channel = 0;
    } else {
        const SrcRecord sr = nd.srec[s]; // (one line: position, power, probability, channel)
        r.x = sr.x;
        r.y = sr.y;
        r.z = sr.z;
        r.txpower = sr.txpower;
        r.txprob = sr.txprob;
        r.start_us = start_us;
        r.air_us = air_us;
        r.src = s;
        r.channel = sr.channel;
    }
    return r;
}

// ---- wave-level helpers

RM_D uint32_t lane_prefix(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
}

RM_D uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// Values that are the same in every lane of a wave but that the compiler cannot know to be (the wave
// index, anything read from LDS or memory at a wave-uniform address): moved to a scalar register,
// so that the loops and branches they steer run on the scalar unit instead of as masked vector code.
RM_D int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
RM_D uint32_t uniform_u(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
RM_D int wave_index() { return __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)); }

// Called by whole waves: the `value` of every lane for which `won` holds is appended to `queue` behind *tail, in lane order, with
// one atomicAdd per wave.  Nothing is stored at or beyond `cap` (the tail still counts such an entry).
__device__ __forceinline__ void wave_append(const bool won, uint32_t *tail, int32_t *queue, const int32_t value, const uint32_t cap, const int lane)
{
    const uint64_t wm = ballot64(won);
    if (!wm) return;
    uint32_t base = 0u;
    if (lane == 0) base = atomicAdd(tail, uint32_t(__popcll(wm)));
    base = uniform_u(base);
    const uint32_t at = base + lane_prefix(wm);
    if (won && at < cap) queue[at] = value;
}

// What a query reports of its final path costs, as each wave of a grid-stride pass over cost[0 .. n) sees it: how many are not
// `unreached`, the largest of those, and how many of them are 0 (the roots).  Every lane returns its wave's figures; the caller
// adds them up with atomics of its own.
struct CostTotals {
    unsigned long long reached, max, zeros;
};
__device__ __forceinline__ CostTotals wave_cost_totals(const unsigned long long *cost, const int n, const unsigned long long unreached)
{
    CostTotals t{0ull, 0ull, 0ull};
    for (int i = int(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += int(gridDim.x * blockDim.x)) {
        const unsigned long long c = cost[i];
        if (c != unreached) {
            ++t.reached;
            t.zeros += c == 0ull;
            t.max = c > t.max ? c : t.max;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        t.reached += __shfl_xor(t.reached, d);
        t.zeros += __shfl_xor(t.zeros, d);
        const unsigned long long o = __shfl_xor(t.max, d);
        t.max = o > t.max ? o : t.max;
    }
    return t;
}

// Consecutive lanes with equal `key` form a run (candidate entries of one frame are contiguous in
// the list).  For the lanes with `pred`: how many such lanes precede me inside my run, how many
// the run has, and which lane leads it -- so that one atomic per run replaces one per link.
struct RunInfo {
    int start;
    uint32_t before, total;
};
RM_D RunInfo run_prefix(int key, bool pred, int lane)
{
    const int prev = __shfl_up(key, 1);
    const uint64_t starts = ballot64(lane == 0 || key != prev);
    const uint64_t preds = ballot64(pred);
    const uint64_t upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull); // lanes 0..lane
    RunInfo r;
    r.start = 63 - __clzll((long long)(starts & upto));
    const uint64_t later = starts & ~upto;
    const int end = later ? (__ffsll((long long)later) - 1) : 64;
    const uint64_t run = ((end == 64) ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << r.start) - 1ull);
    r.before = uint32_t(__popcll(preds & run & ((1ull << lane) - 1ull)));
    r.total = uint32_t(__popcll(preds & run));
    return r;
}

// squared fp32 distance; fma is fine here: the filter only has to be conservative, and the box
// test uses the very same expression (monotone in each |d|)
RM_D float dist2_f32(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

// THE box test of every cull level (receiver group, filter workgroup, block of workgroups, partition): the frame's pre-filter
// record f (position, squared cut-off in w) against a box (x0, y0, x1, y1) / (z0, z1) -- clamped, squared, compared with f.w
RM_D bool box_near(const float4 &qb, const float2 &qz, const float4 &f)
{
    const float dx = fmaxf(fmaxf(qb.x - f.x, f.x - qb.z), 0.f);
    const float dy = fmaxf(fmaxf(qb.y - f.y, f.y - qb.w), 0.f);
    const float dz = fmaxf(fmaxf(qz.x - f.z, f.z - qz.y), 0.f);
    return dist2_f32(dx, dy, dz) <= f.w;
}

// A union of boxes and of the channel masks that go with them (receiver groups -> filter workgroup -> block of workgroups ->
// partition); every level's box contains the boxes below it, so box_near against it is conservative for them.
struct BoxUnion {
    float4 xy; // (x0, y0, x1, y1)
    float2 z;  // (z0, z1)
    uint32_t chmask;
};
RM_D BoxUnion box_union_empty()
{
    const float inf_ = __builtin_inff();
    BoxUnion u;
    u.xy = make_float4(inf_, inf_, -inf_, -inf_);
    u.z = make_float2(inf_, -inf_);
    u.chmask = 0u;
    return u;
}
RM_D void box_union_add(BoxUnion &u, const float4 &q, const float2 &qz, const uint32_t chmask)
{
    u.xy.x = fminf(u.xy.x, q.x);
    u.xy.y = fminf(u.xy.y, q.y);
    u.xy.z = fmaxf(u.xy.z, q.z);
    u.xy.w = fmaxf(u.xy.w, q.w);
    u.z.x = fminf(u.z.x, qz.x);
    u.z.y = fmaxf(u.z.y, qz.y);
    u.chmask |= chmask;
}
// ... over the lanes of a wave: a butterfly at distances d0, d0 / 2, .. 1 (32: the whole wave, 8: every 16 lanes)
RM_D void box_union_lanes(BoxUnion &u, const int d0)
{
#pragma unroll
    for (int d = d0; d >= 1; d >>= 1)
        box_union_add(u, make_float4(__shfl_xor(u.xy.x, d), __shfl_xor(u.xy.y, d), __shfl_xor(u.xy.z, d), __shfl_xor(u.xy.w, d)),
                      make_float2(__shfl_xor(u.z.x, d), __shfl_xor(u.z.y, d)), uint32_t(__shfl_xor(int(u.chmask), d)));
}
// Second level of the sweep on the shadowed medium: with this link's shadowing deviate, can it still reach the level?
// tbl: the conservative table of the largest link hash that can, per bin of rho = s2 / thr (inv: bins / thr of the frame,
// 0: the table is not usable for it -- bin 0 always passes); the hash is of the ordered (source, receiver) pair.
RM_D bool shadow_pass(const ModelDev &m, const uint32_t *tbl, const float s2, const float inv, const int src, const int orig)
{
    const int bin = min(kShadowBins - 1, int(s2 * inv));
    const uint32_t a = uint32_t(src), b = uint32_t(orig);
    const uint64_t key = (uint64_t(a < b ? a : b) << 32) | uint64_t(a < b ? b : a);
    return uint32_t(mix64(m.ld_seed_mixed ^ key) >> 32) <= tbl[bin];
}
// bins / thr of a frame for that table.  It is indexed by rho = s2 / thr: usable if the fp32 frame error is small against
// the distances where it decides anything (d > 0.15 cut), else 0
RM_D float prefilter_inv(const ModelDev &m, const float4 &f)
{
    float inv = 0.f;
    if (m.shadow_tbl && f.w > 0.f && f.w < __builtin_inff()) {
        const double cut = sqrt(double(f.w));
        if (2.0 * m.f32_slack / (0.15 * cut) + 1e-5 <= kShadowPad) inv = float(kShadowBins) / f.w;
    }
    return inv;
}

// What a tick's pre-pass zeroes for the kernels behind it -- the next tick's counters (other parity: nothing touches them
// during this tick), the words later kernels of this tick (cursor) or the next tick's filter (candidate totals) add to, a
// batch's per-receiver link lists or sums -- shared by `stride` threads, this one the `first`-th of them.
RM_D void tick_zero_duties(const TickDev &t, const int first, const int stride)
{
    if (first < 8) t.next_counters[first] = 0u;
    for (int i = first; i < kShards; i += stride) t.next_shard_count[i * kShardStride] = 0u;
    if (!t.use_matrix)
        for (int i = first; i < t.zero_len; i += stride) {
            t.cursor[i] = 0u;
            t.cand_tot_next[i] = 0u;
        }
    if (t.reset_heads) // SINR tick of a batch: every receiver's link list starts empty
        for (int i = first; i < t.n_rx; i += stride) t.head[i] = -1;
    if (t.acc_lo) // ... or, summed per receiver (TickDev::acc_lo): every receiver's sum starts at zero, nobody is on the air yet
        for (int i = first; i < t.n_rx; i += stride) {
            t.acc_lo[i] = 0ull;
            t.acc_hi[i] = 0ull;
        }
}

// The sweep's conservative tests for one (node, frame) pair, shared by the query (k_energy_sum), the gate (k_cca_gate) and the gated batch (rm_ccabatch.hip): same
// channel, not the node's own frame (RM_ED_TRANSMITTING says that it is sending), fp32 distance against the squared cut-off (which
// carries the fp32 frame's slack), the shadowed medium's link-hash table (tbl: its kShadowBins words, staged in LDS).  A node
// outside the frame the fp32 slack was computed for (`wide`) takes every co-channel frame as a candidate.
struct EdNode {
    bool valid, wide, shadow;
    int ch, j;
    float px, py, pz; // position in the fp32 frame
};
RM_D bool ed_candidate(const ModelDev &m, const uint32_t *tbl, const EdNode &nv, const float4 &f, const int4 &fm)
{
    if (!(nv.valid && fm.x == nv.ch && fm.z != nv.j)) return false;
    if (nv.wide) return true;
    const float s2 = dist2_f32(nv.px - f.x, nv.py - f.y, nv.pz - f.z);
    if (!(s2 <= f.w)) return false;
    if (!nv.shadow) return true;
    return shadow_pass(m, tbl, s2, __int_as_float(fm.w), fm.z, nv.j);
}

// a 64-bit sum over the lanes of a wave (the gates add 128-bit Q80 sums limb by limb: integer adds, the order cannot matter)
RM_D unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- one link, the reference's way

struct LinkEval {
    bool append;   // stays in the link list
    bool wanted;   // heard link of a new frame: gets an output record
    uint8_t flags;
    double aux;    // probability (UDGM / N2N) or rssi (logdist)
    double lin;    // linear power (SINR)
};

// Exact evaluation of one link, in the reference's order of tests
// (UDGMRadioMedium.java:99-111, N2NRadioMedium.java:55-67, NullRadioMedium.java:62-73,
//  UDGMConstantLossRadioMedium.java:25-33).  `pos` is the receiver's engine position.
template <int MODEL, bool SINR>
RM_D LinkEval eval_link(const ModelDev &m, const NodesDev &nd, const rm_tx_record &tx, const RxRecord &rx_, bool is_new)
{
    LinkEval r;
    r.append = false;
    r.wanted = false;
    r.flags = 0;
    r.aux = 0.0;
    r.lin = 0.0;
    const int j = rx_.orig;
    if (j == tx.src) return r;                  // node != source
    if (!rx_.enabled) return r;                 // radio.isEnabled()
    if (rx_.channel != tx.channel) return r;    // radio.getWirelessChannel() == channel
    if (MODEL == RM_MODEL_NULL) {
        r.append = r.wanted = is_new;
        r.flags = kFlagHeardNew;
        return r;
    }
    if (MODEL == RM_MODEL_N2N) {
        // N2NRadioMedium.java:28-37
        const int sid = nd.sint_id[tx.src];
        const int did = rx_.int_id;
        double p = 0.0;
        if (m.n2n != nullptr && sid > 0 && did > 0 && sid <= m.n2n_m && did <= m.n2n_m) {
            p = m.n2n[int64_t(sid - 1) * m.n2n_m + (did - 1)] * rx_.rxprob;
        }
        if (p <= 0.0) return r;
        r.append = r.wanted = is_new;
        r.flags = kFlagHeardNew;
        r.aux = p;
        return r;
    }
    const double rx = rx_.x, ry = rx_.y, rz = rx_.z;
    if (MODEL == RM_MODEL_UDGM_CONST) {
        const double d = ref_distance(tx.x, tx.y, tx.z, rx, ry, rz);
        if (d < m.const_range) {
            r.append = r.wanted = is_new;
            r.flags = kFlagHeardNew;
        }
        return r;
    }
    if (MODEL == RM_MODEL_UDGM) {
        // UDGMRadioMedium.java:67-81 ; Math.pow(v, 2.0) == v*v
        const double d = ref_distance(tx.x, tx.y, tx.z, rx, ry, rz);
        const double d2 = d * d;
        const double dmax = m.udgm_range;
        if (dmax == 0.0) return r;
        const double dmax2 = dmax * dmax;
        double ratio = d2 / dmax2;
        if (ratio > 1.0) return r;
        ratio = 1.0 - ratio * (1.0 - m.udgm_ratio_rx);
        const double p = ratio * rx_.rxprob;
        if (p <= 0.0) return r;
        r.append = r.wanted = is_new;
        r.flags = kFlagHeardNew;
        r.aux = p;
        return r;
    }
    if (MODEL == RM_MODEL_LOGDIST) {
        const double rssi = logdist_rssi(m, tx, rx, ry, rz, j);
        const bool heard = is_new && (rssi >= m.ld_sens) && !(rx_.rxprob <= 0.0);
        r.aux = rssi;
        if (SINR) {
            const bool interferer = rssi >= m.ld_ifloor;
            if (!heard && !interferer) return r;
            r.append = true;
            r.wanted = heard;
            r.flags = uint8_t((heard ? kFlagHeardNew : 0) | (interferer ? kFlagInterferer : 0));
            if (interferer) r.lin = det_pow10(rssi / 10.0);
        } else if (heard) {
            r.append = r.wanted = true;
            r.flags = kFlagHeardNew;
        }
        return r;
    }
    return r;
}

// Exclusive scan of n per-frame counts inside one 256-thread workgroup, result in LDS (and in
// `pub` if not null).  Every workgroup of a consumer kernel redoes it (T counts, a few KB from L2)
// instead of paying a separate kernel for it.  Returns the total; *vmax gets the largest count.
RM_D uint32_t block_scan_counts(const uint32_t *cnt, int n, uint32_t *s_off, uint32_t *s_wave /*[4]*/, uint32_t *pub,
                                uint32_t *vmax_out)
{
    const int per = (n + 255) / 256;
    const int i0 = min(n, int(threadIdx.x) * per), i1 = min(n, i0 + per);
    uint32_t sum = 0, vmax = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t v = cnt[i];
        sum += v;
        vmax = max(vmax, v);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
    const uint32_t total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    for (int i = i0; i < i1; ++i) {
        s_off[i] = run;
        if (pub) pub[i] = run;
        run += cnt[i];
    }
    if (pub && threadIdx.x == 0) pub[n] = total;
    if (threadIdx.x == 0) s_off[n] = total; // (a consumer takes a frame's count as the difference of two offsets)
    if (vmax_out) {
        for (int d = 32; d >= 1; d >>= 1) vmax = max(vmax, uint32_t(__shfl_xor(int(vmax), d)));
        *vmax_out = vmax;
    }
    __syncthreads();
    return total;
}

// The same for at most 256*PER counts (PER = 4: the bench's 1000 frames per tick, 16: up to 4096):
// PER counts per thread, requested with small_scan_load at the top of the kernel so that the
// round trip overlaps the kernel's own first loads, and only 1 KB * PER of LDS (the occupancy of
// the consumers is LDS-bound with the general 32 KB variant).
constexpr int kSmallScan = 1024, kMediumScan = 4096;
template <int PER> struct SmallCounts {
    uint32_t v[PER];
};
template <int PER> RM_D SmallCounts<PER> small_scan_load(const uint32_t *cnt, int n)
{
    SmallCounts<PER> c;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = int(threadIdx.x) * PER + k;
        c.v[k] = (i < n) ? cnt[i] : 0u;
    }
    return c;
}
template <int PER>
RM_D uint32_t small_scan(const SmallCounts<PER> &c, int n, uint32_t *s_off, uint32_t *s_wave /*[4]*/, uint32_t *pub, uint32_t *vmax_out)
{
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) sum += c.v[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
    const uint32_t total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = int(threadIdx.x) * PER + k;
        if (i < n) {
            s_off[i] = run;
            if (pub) pub[i] = run;
        }
        run += c.v[k];
    }
    if (pub && threadIdx.x == 0) pub[n] = total;
    if (threadIdx.x == 0) s_off[n] = total;
    if (vmax_out) {
        uint32_t vmax = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) vmax = max(vmax, c.v[k]);
        for (int d = 32; d >= 1; d >>= 1) vmax = max(vmax, uint32_t(__shfl_xor(int(vmax), d)));
        // the publisher needs the maximum over the whole workgroup
        __shared__ uint32_t s_vmax[4];
        if (lane == 0) s_vmax[wave] = vmax;
        __syncthreads();
        *vmax_out = max(max(s_vmax[0], s_vmax[1]), max(s_vmax[2], s_vmax[3]));
    }
    __syncthreads();
    return total;
}
// scan variant of a kernel template parameter: 1 general (<= kFusedScanMax), 3 small, 4 medium
constexpr int scan_per(int v) { return v == 3 ? 4 : 16; }
constexpr int scan_lds(int v) { return v == 1 ? kFusedScanMax + 1 : (v == 3 ? kSmallScan + 1 : (v == 4 ? kMediumScan + 1 : 1)); }
static inline int scan_variant(int n_cnt) { return n_cnt <= kSmallScan ? 3 : (n_cnt <= kMediumScan ? 4 : (n_cnt <= kFusedScanMax ? 1 : 2)); }

RM_D double tx_success(const ModelDev &m, const rm_tx_record &tx)
{
    // UDGMRadioMedium.java:63-65 uses successRatioRx (sic); N2NRadioMedium.java:24-26
    if (m.kind == RM_MODEL_UDGM) return m.udgm_ratio_rx * tx.txprob;
    return tx.txprob;
}

// ---- 1024-thread scans

RM_D uint32_t wave_inclusive_scan(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// ---- a wave's 64 runs copied with full lanes (the heard form's two record copies: k_reorder_served_batch, k_nc_fill_batch)
// The index rule, host-callable (tests/cpp/wave_runs_san_test.cpp holds it to a plain expansion of the runs): the entries
// j = 0 .. total - 1 of the runs laid end to end are taken a SPAN of kCopyRounds * 64 at a time, entry j0 + 64 u + lane by
// `lane` in round u -- every entry exactly once.
constexpr int kCopyRounds = 4;
constexpr uint32_t kCopySpan = 64u * kCopyRounds;
// the run that holds entry j: the first one whose running count is above j (63 for a j at or beyond the total) -- wave_run_of's
// bisection over any way of reading run i's running count (the host: an array; the wave: a lane's register)
template <class IncAt>
RM_HD int run_of(const IncAt inc_at, const uint32_t j)
{
    int lo = 0, hi = 63;
#pragma unroll
    for (int step = 0; step < 6; ++step) {
        const int mid = (lo + hi) >> 1;
        const bool above = inc_at(mid) > j;
        hi = above ? mid : hi;
        lo = above ? lo : mid + 1;
    }
    return lo < 63 ? lo : 63;
}
// entry j's place in its run (the run's running count and length)
RM_HD uint32_t run_place(const uint32_t run_inc, const uint32_t run_cnt, const uint32_t j) { return j - (run_inc - run_cnt); }
// the lanes' runs (inc: wave_inclusive_scan of their lengths): the lane whose run holds entry j
RM_D int wave_run_of(const uint32_t inc, const uint32_t j)
{
    return run_of([inc](const int i) { return uint32_t(__shfl(int(inc), i)); }, j);
}

// The copy itself.  Lane f's run: cnt records (inc: wave_inclusive_scan of cnt, total: the wave's sum), at list0 in the arena's
// columns and at rec0 in the tick's ordered records.  TO_ARENA: records -> arena (a claimed list is filled), else arena -> records
// (a hit frame is served; out_pkt is written as well: frame e0 + f).  kCopyRounds rounds of 64 entries at a time, all their loads
// requested before the first store (the arena and the records may alias as far as the compiler knows, so it would wait for every
// round's loads on its own).  Every access is guarded: both ends are memory that all ticks of the batch share.
template <bool TO_ARENA>
RM_D void wave_copy_lists(const TickDev &t, const int lane, const int e0, const uint32_t cnt, const uint32_t inc, const uint32_t total,
                          const uint32_t list0, const uint32_t rec0)
{
    for (uint32_t j0 = 0; j0 < total; j0 += kCopySpan) { // wave-uniform
        uint32_t a[kCopyRounds], o[kCopyRounds];
        bool ok[kCopyRounds];
        int pkt[kCopyRounds], v_dst[kCopyRounds];
        double v_rssi[kCopyRounds];
        uint8_t v_verdict[kCopyRounds];
#pragma unroll
        for (int u = 0; u < kCopyRounds; ++u) {
            const uint32_t j = j0 + uint32_t(u * 64 + lane);
            const int f = wave_run_of(inc, j);
            const uint32_t f_inc = uint32_t(__shfl(int(inc), f)), f_cnt = uint32_t(__shfl(int(cnt), f));
            const uint32_t k = run_place(f_inc, f_cnt, j);
            a[u] = uint32_t(__shfl(int(list0), f)) + k;
            o[u] = uint32_t(__shfl(int(rec0), f)) + k;
            pkt[u] = e0 + f;
            ok[u] = j < total && o[u] < t.cap && a[u] < t.nc.arena_len;
            if (TO_ARENA) {
                v_dst[u] = ok[u] ? t.out_dst[o[u]] : 0;
                v_rssi[u] = ok[u] ? t.out_rssi[o[u]] : 0.0;
                v_verdict[u] = ok[u] ? t.out_verdict[o[u]] : uint8_t(0);
            } else {
                v_dst[u] = ok[u] ? t.nc.arena[a[u]] : 0;
                v_rssi[u] = ok[u] ? t.nc.arena_rssi[a[u]] : 0.0;
                v_verdict[u] = ok[u] ? t.nc.arena_verdict[a[u]] : uint8_t(0);
            }
        }
#pragma unroll
        for (int u = 0; u < kCopyRounds; ++u) {
            if (!ok[u]) continue;
            if (TO_ARENA) {
                t.nc.arena[a[u]] = v_dst[u];
                t.nc.arena_rssi[a[u]] = v_rssi[u];
                t.nc.arena_verdict[a[u]] = v_verdict[u];
            } else {
                t.out_pkt[o[u]] = pkt[u];
                t.out_dst[o[u]] = v_dst[u];
                t.out_rssi[o[u]] = v_rssi[u];
                t.out_verdict[o[u]] = v_verdict[u];
            }
        }
    }
}

// exclusive scan of one value per thread over a 1024-thread block; returns the block total in `total`
RM_D uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t *s_wave /*[16]*/, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t wave_off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const uint32_t x = s_wave[w];
        if (w < wave) wave_off += x;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return wave_off + inc - v;
}

// per-packet Tx-failure flag where no draw can happen (txSuccess <= 0 is the only way to fail)
// ---- the on-air lists across ticks (AirDev, rm_engine.h)
// room for the wanted lanes' entries in sub-ring `sub`: one atomic per wave.  Whole waves call this together.
RM_D int air_alloc(const TickDev &t, bool want, uint32_t sub)
{
    const unsigned long long mask = __ballot(want);
    if (mask == 0ull) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    const uint32_t cnt = uint32_t(__popcll(mask));
    uint32_t base = 0;
    if (lane == leader) {
        base = atomicAdd(&t.air.tail[sub * kShardStride], cnt);
        const uint32_t live0 = t.air.mark[(t.air.wtick & (kAirTicks - 1)) * kShards + sub];
        if (base + cnt - live0 > t.air.sub_mask + 1u) { // would overwrite entries of frames still on the air
            t.stage_count[1] = 1u;
            t.air.bad[0] = 1u; // sticky: every later tick is dropped as well until the host has rebuilt the lists
        }
    }
    base = uint32_t(__shfl(int(base), leader));
    if (!want) return -1;
    const uint32_t seq = base + uint32_t(__popcll(mask & ((1ull << lane) - 1ull)));
    return int((sub << t.air.sub_shift) | (seq & t.air.sub_mask));
}

RM_D uint32_t air_sub(const TickDev &t)
{
    return (blockIdx.x * 4u + (threadIdx.x >> 6) + blockIdx.y * 17u + t.air.tick * 61u) & uint32_t(kShards - 1);
}

// the entry becomes the head of its receiver's list; the old head is kept as `next` only if it is still live
RM_D void air_link(const TickDev &t, int aidx, int pos, int64_t start_us, int64_t air_us, double lin, uint32_t flags)
{
    const unsigned long long mine = ((unsigned long long)t.air.tick << 32) | uint32_t(aidx);
    const unsigned long long old = atomicExch(&t.air.head[pos], mine);
    AirEntry e;
    e.start_us = start_us;
    e.lin = lin;
    e.air_us = uint32_t(air_us);
    if ((unsigned long long)air_us >> 32) { // (records in device memory are not seen by the host: a frame of 2^32 us or more)
        t.stage_count[1] = 1u;
        t.air.bad[0] = 1u;
    }
    e.next = (uint32_t(old >> 32) >= t.air.wtick) ? int(uint32_t(old)) : -1; // an empty head has tick 0
    e.meta = (t.air.tick << 2) | flags;
    e.pad = 0u;
    t.air.pool[aidx] = e;
}

// The tick is over for the lists: the next tick's entries begin where the sub-rings' tails are now.  One workgroup of
// kShards threads, after the last allocation of the tick (a later kernel than the one that evaluates the links).
RM_D void air_end(const TickDev &t)
{
    if (threadIdx.x < uint32_t(kShards))
        t.air.mark[((t.air.tick + 1u) & (kAirTicks - 1)) * kShards + threadIdx.x] = t.air.tail[threadIdx.x * kShardStride];
}

struct SinrOut {
    double sinr;
    bool collided;
};

// SINR of one heard link of a new frame (start w_start, length w_air) at the receiver in engine position `pos`: the
// receiver's list holds every co-channel frame on the air that is significant there; the interferers that overlap the
// frame in time are summed exactly (Q80: the order of the list does not matter), a SELF entry is half duplex.
// `self` is the link's own entry -- or kAirOwnInSum when the caller does not know it: the link's own entry is then
// summed like every other and taken out again afterwards, which is exact in Q80 (the entry exists iff the link is an
// interferer itself, rssi >= ifloor, and it is counted iff the frame overlaps itself and has not left the air).
constexpr int kAirOwnInSum = -2;
RM_D SinrOut air_sinr(const ModelDev &m, const TickDev &t, int pos, int self, int64_t w_start, int64_t w_air, double rssi)
{
    U128 acc = {0, 0};
    bool half_duplex = false;
    const int64_t w_end = w_start + w_air;
    const unsigned long long h = t.air.head[pos];
    uint32_t prev = uint32_t(h >> 32);
    int idx = (prev >= t.air.wtick) ? int(uint32_t(h)) : -1;
    for (int hops = 0; idx >= 0 && hops < (1 << 22); ++hops) {
        const AirEntry k = t.air.pool[idx];
        const uint32_t kt = k.meta >> 2;
        if (kt > prev || kt < t.air.wtick) break; // a slot that was handed out again: the list ended before it
        prev = kt;
        const int64_t k_end = k.start_us + int64_t(k.air_us);
        if (idx != self && k_end > t.air.t_begin && k.start_us < w_end && k_end > w_start) {
            if (k.meta & kAirSelf) half_duplex = true;
            else acc = u128_add(acc, q80_from_double(k.lin));
        }
        idx = k.next;
    }
    if (self == kAirOwnInSum && rssi >= m.ld_ifloor && w_air > 0 && w_end > t.air.t_begin)
        acc = u128_sub(acc, q80_from_double(det_pow10(rssi / 10.0))); // eval_link's lin of this very link
    SinrOut r;
    r.sinr = rssi - 10.0 * det_log10(q80_to_double(acc) + m.ld_noise_lin);
    r.collided = half_duplex || !(r.sinr >= m.ld_capture);
    return r;
}

RM_D void write_pkt_interference(const ModelDev &m, const TickDev &t, uint32_t first, uint32_t stride)
{
    const bool draws_possible = (m.kind == RM_MODEL_UDGM || m.kind == RM_MODEL_N2N || m.kind == RM_MODEL_LOGDIST);
    const int n_new = t.n_active - t.first_new;
    for (uint32_t q = first; q < uint32_t(n_new); q += stride) {
        const rm_tx_record tx = t.tx[t.first_new + q];
        t.pkt_interference[q] = (draws_possible && tx_success(m, tx) <= 0.0) ? 1 : 0;
    }
}

// the smallest fused-scan variant that holds every tick's counts
static inline int batch_scan_variant(const TickDev *ticks, int n)
{
    int scan = 3;
    for (int i = 0; i < n; ++i) {
        const int v = scan_variant(ticks[i].n_cnt);
        scan = (v == 1 || scan == 1) ? 1 : max(scan, v);
    }
    return scan;
}

// ---- what the gated batch (rm_ccabatch.hip) and the CSMA-CA gated batch (rm_csma.hip) share: the index entry of one frame, one
// wave's walk over the indexed frames within its node's reach, the wave's 128-bit sum

// live at t: start <= t < start + air (the end of a span is exclusive; the query's test)
RM_D bool cb_live(int64_t t, int64_t start_us, int64_t air_us) { return !(t < start_us || t - start_us >= air_us); }

// frame f (record r, of tick tk; -1: a window frame) joins its source node's chain and the grid or the EVERY list; CHAIN_ALL: a frame
// that is never live joins the chain too (the CSMA-CA batch finds a node's slots of one tick there)
template <bool GRID, bool CHAIN_ALL = false>
RM_D void cb_index_frame(const NodesDev &nd, const ModelDev &m, const CcaBatchDev &cb, const int f, const rm_tx_record &r, const int tk)
{
    if (!CHAIN_ALL && r.air_us <= 0) return; // (never live)
    if (r.src < nd.n) {
        const unsigned long long stamp = (unsigned long long)cb.stamp << 32;
        const unsigned long long old = atomicExch(&cb.self_slot[r.src], stamp | (unsigned long long)uint32_t(f));
        cb.self_next[f] = (uint32_t(old >> 32) == cb.stamp) ? int(uint32_t(old)) : -1;
    }
    if (CHAIN_ALL && r.air_us <= 0) return;
    float4 p;
    double thr64;
    tx_prefilter_at(m, m.ld_ifloor, r, p, thr64);
    if (!(p.w >= 0.f)) return; // reaches the floor nowhere
    float inv = 0.f;           // squared fp32 distance -> bin of the link-hash table (k_energy_index)
    if (m.shadow_tbl != nullptr && p.w > 0.f && p.w < __builtin_inff()) {
        const float cut = __builtin_sqrtf(p.w);
        if (1.01f * (2.0f * float(m.f32_slack)) / (0.15f * cut) + 1e-5f <= float(kShadowPad)) inv = float(kShadowBins) / p.w;
    }
    const int4 meta = make_int4(r.channel, f, r.src, __float_as_int(inv));
    if (GRID && p.w < __builtin_inff()) {
        const int cell = sg_cell1(p.y, cb.half, cb.inv) * kEdG + sg_cell1(p.x, cb.half, cb.inv);
        atomicMax(&cb.cnt[1], __float_as_uint(sqrt_up(p.w)));
        const uint32_t k = atomicAdd(&cb.cnt[2 + cell], 1u);
        if (k < uint32_t(kCbK)) {
            cb.bucket_f[cell * kCbK + int(k)] = p;
            cb.bucket_m[cell * kCbK + int(k)] = meta;
            cb.bucket_t[cell * kCbK + int(k)] = tk;
            return;
        }
    }
    const uint32_t e = atomicAdd(&cb.cnt[0], 1u); // (at most one entry per frame: the list has room for every frame)
    cb.every_f[e] = p;
    cb.every_m[e] = meta;
    cb.every_t[e] = tk;
}

// one wave, a node at (px, py) of the fp32 frame: look(entry, meta, tick) for every frame of the grid's cells within reach and of
// the EVERY list, a lane per frame.  w_off[65] / w_cell[64]: the wave's own words of LDS.
template <bool GRID, class Look>
RM_D void cb_walk(const CcaBatchDev &cb, int *w_off, int *w_cell, const int lane, const bool wide, const float px, const float py, Look &&look)
{
    if (GRID) {
        // the cells that can hold a frame within reach (as the query: |dx| <= largest radius, positions map to cells monotonically)
        const float rmax = __uint_as_float(cb.cnt[1]);
        const float reach = rmax * (1.0f + 2e-5f) + 1e-3f / cb.inv;
        int cx0 = 0, cy0 = 0, cx1 = kEdG - 1, cy1 = kEdG - 1;
        if (!wide) {
            cx0 = sg_cell1(px - reach, cb.half, cb.inv);
            cx1 = sg_cell1(px + reach, cb.half, cb.inv);
            cy0 = sg_cell1(py - reach, cb.half, cb.inv);
            cy1 = sg_cell1(py + reach, cb.half, cb.inv);
        }
        cx0 = uniform_i(cx0), cx1 = uniform_i(cx1), cy0 = uniform_i(cy0), cy1 = uniform_i(cy1);
        const int ncx = cx1 - cx0 + 1, ncells = ncx * (cy1 - cy0 + 1);
        for (int c0 = 0; c0 < ncells; c0 += 64) { // wave-uniform
            const int c = c0 + lane;
            int cell = 0, cnt = 0;
            if (c < ncells) {
                cell = (cy0 + c / ncx) * kEdG + cx0 + c % ncx;
                cnt = int(min(cb.cnt[2 + cell], uint32_t(kCbK))); // every cell's count at once
            }
            int incl = cnt; // inclusive prefix over the wave
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            const int total = uniform_i(__shfl(incl, 63));
            if (total == 0) continue;
            w_off[lane] = incl - cnt;
            w_cell[lane] = cell;
            if (lane == 63) w_off[64] = total;
            __builtin_amdgcn_wave_barrier(); // (LDS traffic of one wave is in order; the compiler must not move it either)
            for (int e = lane; e < total; e += 64) { // the entries, whichever cell they are in
                int lo = 0;                              // the last cell whose first entry is <= e
                for (int step = 32; step > 0; step >>= 1)
                    if (w_off[lo + step] <= e) lo += step;
                const int at = w_cell[lo] * kCbK + (e - w_off[lo]);
                look(cb.bucket_f[at], cb.bucket_m[at], cb.bucket_t[at]);
            }
            __builtin_amdgcn_wave_barrier(); // (the next round rewrites the offsets)
        }
    }
    const int n_every = uniform_i(int(cb.cnt[0]));
    for (int e = lane; e < n_every; e += 64) look(cb.every_f[e], cb.every_m[e], cb.every_t[e]);
}

// the wave's sum of 128-bit values: four 32-bit limbs, each added across the lanes in 64 bits, carries once (k_cca_gate); mod 2^128,
// as the query's sums
RM_D U128 wave_sum_u128(const U128 acc)
{
    const unsigned long long l0 = wave_sum_u64(acc.lo & 0xFFFFFFFFull), l1 = wave_sum_u64(acc.lo >> 32);
    const unsigned long long l2 = wave_sum_u64(acc.hi & 0xFFFFFFFFull), l3 = wave_sum_u64(acc.hi >> 32);
    __builtin_amdgcn_wave_barrier();
    U128 sum, part;
    sum.lo = l0, sum.hi = l2;
    part.lo = l1 << 32, part.hi = (l1 >> 32) + (l3 << 32);
    return u128_add(sum, part);
}

// ---- a finished result slot's answer about (packet p, wanted node w): the unicast query's status (E12) and the link's index.  What
// rm_unicast.hip writes out per entry and what the forwarding queues' advance (rm_fwd.hip) decides an attempt by
RM_D bool uc_lost(const UcSlot &s) { return s.out_count[1] != 0u || (s.stage_count && s.stage_count[1] != 0u); }

RM_D int uc_find(const UcSlot &s, int p, int w, int n_nodes, int32_t &link)
{
    int status = RM_UC_NONE;
    link = -1;
    if (w >= 0 && p >= 0 && p < s.n_new && s.out_count && s.recs) {
        if (uc_lost(s)) {
            status = RM_UC_LOST; // the traffic counters' skip condition (rm_stats.hip)
        } else {
            const int32_t src = s.recs[p].src;
            if (src < 0 || src >= n_nodes) {
                status = RM_UC_NOT_SENT;
            } else {
                status = RM_UC_UNHEARD;
                if (s.pkt_offset && s.dst && s.verdict) {
                    const uint32_t n = min(s.out_count[0], s.out_count[2]); // (never past the links that were stored)
                    const uint32_t end = min(s.pkt_offset[p + 1], n);
                    uint32_t lo = min(s.pkt_offset[p], end), hi = end;
                    while (lo < hi) { // lower bound of w in dst[lo, hi)
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        if (s.dst[mid] < w) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo < end && s.dst[lo] == w) {
                        link = int32_t(lo);
                        status = s.verdict[lo] == uint8_t(RM_DELIVERED) ? RM_UC_DELIVERED : RM_UC_INTERFERED;
                    }
                }
            }
        }
    }
    return status;
}

// ---- what the kernels of the node-table features share: the traffic generator's scan (rm_traffic.hip) and all of the following
// for the relay features, which are driven by a finished result slot (rm_fwd.hip, rm_flood.hip)
using u64 = unsigned long long;
constexpr int kRelayThreads = 256;
inline int relay_blocks(int n) { return std::max(1, (n + kRelayThreads - 1) / kRelayThreads); } // (host: workgroups for n lanes)

RM_D u64 *relay_w(uint64_t *p) { return reinterpret_cast<u64 *>(p); }
template <typename Dev> RM_D bool relay_in(const Dev &f, int j) { return j >= 0 && j < f.n_nodes; }
RM_D bool relay_slot_lost(const UcSlot &s) { return s.out_count && uc_lost(s); }

// the slot's links: stored ones only, and none behind the last packet's segment
RM_D uint32_t relay_links(const UcSlot &s)
{
    if (!s.out_count || !s.pkt_offset || !s.dst || !s.verdict || !s.recs || s.n_new <= 0) return 0u;
    return min(min(s.out_count[0], s.out_count[2]), s.pkt_offset[s.n_new]);
}
// the packet of link i < pkt_offset[n_new]: the last p with pkt_offset[p] <= i (empty packets share their offset with the next one)
RM_D int relay_pkt(const UcSlot &s, const uint32_t i)
{
    int lo = 0, hi = s.n_new;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (s.pkt_offset[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the wave's share of a total -- one address for everybody -- added once
RM_D void relay_total(uint64_t *word, u64 v)
{
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63u) == 0u && v != 0ull) atomicAdd(relay_w(word), v);
}
RM_D void relay_total_max(uint64_t *word, u64 v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u64 o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63u) == 0u && v != 0ull) atomicMax(relay_w(word), v);
}

// The scan of an ordered stream compaction, one 256-thread workgroup per list: the first wave turns the units' counts -- col[u * W],
// a column of unit_count [units][W] -- into exclusive prefixes in place, 64 units at a time, and writes their sum to *out_count;
// then all four waves pad the list behind min(sum, cap) with -1
RM_D void units_scan(const int units, const int W, const int cap, int32_t *col, int32_t *row, int32_t *out_count)
{
    __shared__ int32_t s_total;
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        uint32_t carry = 0;
        for (int u0 = 0; u0 < units; u0 += 64) {
            const int u = u0 + lane;
            const uint32_t v = u < units ? uint32_t(col[size_t(u) * W]) : 0u;
            const uint32_t inc = wave_inclusive_scan(v, lane);
            if (u < units) col[size_t(u) * W] = int32_t(carry + inc - v);
            carry += __shfl(inc, 63);
        }
        if (lane == 0) {
            s_total = int32_t(carry);
            *out_count = int32_t(carry);
        }
    }
    __syncthreads();
    for (int p = min(s_total, cap) + int(threadIdx.x); p < cap; p += 256) row[p] = -1;
}

// The walk of a single source list, before (count) and behind (WRITE) that scan: the node table cut into units of `chunk`
// consecutive nodes, one wave per unit, one lane per node, 64 nodes a round.  member(node) -- called exactly once per node of
// the table and pass -- says whether the node is in the list.  count: unit_count[unit] = the unit's members; WRITE: the members
// go to out_src in ascending order from the unit's prefix on, clipped at cap
template <bool WRITE, typename Member>
RM_D void source_walk(const int n_nodes, const int cap, const int chunk, int32_t *unit_count, int32_t *out_src, Member member)
{
    const int lane = threadIdx.x;
    const int unit = blockIdx.x;
    const int first = unit * chunk;
    const int last = min(first + chunk, n_nodes);
    int run = WRITE ? unit_count[unit] : 0; // WRITE: where the unit's next source goes; else its sources so far
    for (int i0 = first; i0 < last; i0 += 64) {
        const int node = i0 + lane;
        const bool hit = node < last && member(node);
        const uint64_t m = ballot64(hit);
        if (WRITE) {
            const int pos = run + int(lane_prefix(m));
            if (hit && pos < cap) out_src[pos] = node;
        }
        run += __popcll(m);
    }
    if (!WRITE && lane == 0) unit_count[unit] = run;
}

// The first launch of an advance, lane p of P: a lost slot is counted once and nothing else happens (kClaimNone, as for p >= P);
// else the candidate -- cand[p], or the frame's source -- claims its first occurrence by atomicMin of p over claim[j] if it is a
// participant(j) inside the table, and is -1 (foreign traffic) if not.  The caller stores the answer in its own record of p
constexpr int32_t kClaimNone = INT32_MIN;
template <typename Dev, typename Participant>
RM_D int32_t relay_claim(const Dev &f, const UcSlot &s, const int32_t *cand, const int P, const int p, Participant participant)
{
    if (relay_slot_lost(s)) {
        if (p == 0) atomicAdd(relay_w(&f.totals->skipped_slots), 1ull);
        return kClaimNone;
    }
    if (p >= P) return kClaimNone;
    const int32_t j = cand ? cand[p] : s.recs[p].src;
    if (!relay_in(f, j) || !participant(j)) return -1;
    atomicMin(&f.claim[j], p);
    return j;
}

} // namespace rm
