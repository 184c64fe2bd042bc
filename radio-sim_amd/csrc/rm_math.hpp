// rm_math.hpp -- the exact-arithmetic layer: E-math of the extension spec, link hash, Q80 fixed point, java.util.Random
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
#pragma once

#include "rm_engine.h"

#include <math.h>

namespace rm {

#define RM_HD __host__ __device__ inline
#define RM_D __device__ inline

// ============================================================================ exact math
// Extension spec "E-math" (DESIGN.md): + - * / sqrt floor and integer operations only.

RM_HD uint64_t f2u(double d) { return __builtin_bit_cast(uint64_t, d); }
RM_HD double u2f(uint64_t u) { return __builtin_bit_cast(double, u); }

RM_HD double det_log2(double x)
{
    const uint64_t b = f2u(x);
    int e = int((b >> 52) & 0x7FFu) - 1023;
    double m = u2f((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    if (m > 1.4142135623730951) {
        m = m * 0.5;
        e += 1;
    }
    const double f = (m - 1.0) / (m + 1.0);
    const double s = f * f;
    // atanh series: sum_{k=1..11} s^k / (2k+1), highest order first
    double q = 1.0 / 23.0;
#pragma unroll
    for (int k = 10; k >= 1; --k) {
        q = q * s + 1.0 / double(2 * k + 1);
    }
    q = q * s;
    const double r = f + f * q;
    return double(e) + (2.0 * r) * 1.4426950408889634;
}

RM_HD double det_exp2(double y)
{
    if (y != y) return y;
    if (!(y >= -1022.0)) return 0.0;
    if (y > 1023.0) return u2f(0x7FF0000000000000ull);
    const double k = floor(y + 0.5);
    const double r = y - k;
    const double t = r * 0.6931471805599453;
    // exp(t) = sum t^n / n!, n = 13 .. 0
    const double inv_fact[14] = {1.0, 1.0, 0.5, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0,
                                 1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0,
                                 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double q = inv_fact[13];
#pragma unroll
    for (int n = 12; n >= 0; --n) {
        q = q * t + inv_fact[n];
    }
    const double scale = u2f(uint64_t(int64_t(k) + 1023) << 52);
    return q * scale;
}

RM_HD double det_log10(double x) { return det_log2(x) * 0.30102999566398120; }
RM_HD double det_pow10(double y) { return det_exp2(y * 3.3219280948873622); }

// Acklam's rational approximation of the standard normal quantile
RM_HD double det_normal(double u)
{
    const double a1 = -3.969683028665376e+01, a2 = 2.209460984245205e+02, a3 = -2.759285104469687e+02,
                 a4 = 1.383577518672690e+02, a5 = -3.066479806614716e+01, a6 = 2.506628277459239e+00;
    const double b1 = -5.447609879822406e+01, b2 = 1.615858368580409e+02, b3 = -1.556989798598866e+02,
                 b4 = 6.680131188771972e+01, b5 = -1.328068155288572e+01;
    const double c1 = -7.784894002430293e-03, c2 = -3.223964580411365e-01, c3 = -2.400758277161838e+00,
                 c4 = -2.549732539343734e+00, c5 = 4.374664141464968e+00, c6 = 2.938163982698783e+00;
    const double d1 = 7.784695709041462e-03, d2 = 3.224671290700398e-01, d3 = 2.445134137142996e+00,
                 d4 = 3.754408661907416e+00;
    // Branch-free: the central expression and the tail expression are both evaluated and one is selected --
    // operation for operation what the extension spec writes as three cases (the upper tail is the lower
    // tail's expression on 1 - u with the sign flipped).  A wave almost always holds lanes of the centre AND
    // of a tail (4.85 % of the deviates are tail values), so divergent branches would be issued one after
    // the other anyway; as one basic block the two dependent chains (and the caller's distance logarithm)
    // interleave, which is what a latency-bound evaluation -- one frame per workgroup, rm_tick.hip -- needs.
    const bool lower = u < 0.02425;
    const bool tail = lower || !(u <= 0.97575);
    const double t = tail ? (lower ? u : 1.0 - u) : 0.5; // (any value with a finite logarithm for the lanes that discard it)
    const double qt = sqrt(-2.0 * (det_log2(t) * 0.6931471805599453));
    const double rt = (((((c1 * qt + c2) * qt + c3) * qt + c4) * qt + c5) * qt + c6) /
                      ((((d1 * qt + d2) * qt + d3) * qt + d4) * qt + 1.0);
    const double q = u - 0.5;
    const double r = q * q;
    const double rc = (((((a1 * r + a2) * r + a3) * r + a4) * r + a5) * r + a6) * q /
                      (((((b1 * r + b2) * r + b3) * r + b4) * r + b5) * r + 1.0);
    return tail ? (lower ? rt : -rt) : rc;
}

RM_HD uint64_t mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}


// per-link shadowing deviate: symmetric in (a, b), independent of evaluation order / sharding
RM_HD double shadow_gauss(uint64_t seed_mixed, double clip, uint32_t a, uint32_t b)
{
    const uint32_t lo = a < b ? a : b;
    const uint32_t hi = a < b ? b : a;
    const uint64_t h = mix64(seed_mixed ^ ((uint64_t(lo) << 32) | uint64_t(hi)));
    const double u = (double(h >> 12) + 0.5) * 0x1.0p-52;
    double g = det_normal(u);
    if (g > clip) g = clip;
    if (g < -clip) g = -clip;
    return g;
}

// ---- frame error model (extension spec E10): packet success ratio of an 802.15.4 O-QPSK frame and the link's draw ----
// ber = 8/15 * 1/16 * sum_{k=2..16} (-1)^k C(16,k) exp(20 s (1/k - 1)), s the linear SINR; psr = (1 - ber)^bits.
// Every operation is one IEEE rounding in the order DESIGN.md section 6 (E10) writes them; the loop is unrolled, so the
// binomials and the 1/k - 1 are literals of the instruction stream (folded by the compiler with IEEE rounding), not loads.
RM_HD double em_ber_oqpsk(double s)
{
    const double binom[17] = {1.0, 16.0, 120.0, 560.0, 1820.0, 4368.0, 8008.0, 11440.0, 12870.0,
                              11440.0, 8008.0, 4368.0, 1820.0, 560.0, 120.0, 16.0, 1.0};
    const double s20 = 20.0 * s;
    double acc = 0.0;
#pragma unroll
    for (int k = 2; k <= 16; ++k) {
        const double ck = 1.0 / double(k) - 1.0;
        const double yk = (s20 * ck) * 1.4426950408889634;
        const double tk = binom[k] * det_exp2(yk);
        acc = (k & 1) ? acc - tk : acc + tk;
    }
    double ber = acc / 30.0;
    if (ber < 0.0) ber = 0.0;
    if (0.5 < ber) ber = 0.5;
    return ber; // (a NaN passes both comparisons and stays NaN)
}

RM_HD double em_psr_oqpsk(double us_per_bit, double sinr_db, int64_t air_us)
{
    const double s = det_pow10(sinr_db / 10.0);
    const double ber = em_ber_oqpsk(s);
    if (ber != ber) return ber; // (det_log2 reads a NaN's bits as a number: the NaN is handed through here, and never delivers)
    const double n = double(air_us) / us_per_bit;
    return det_exp2(n * det_log2(1.0 - ber));
}

// the route query's link cost: ETX in units of 1/128 from the link's rssi alone -- the text the kernels
// (rm_routes.hip) and rm_routes_link_cost / rm_routes_from_links are both built from.  noise_db = 10 * det_log10(ld_noise_lin),
// max_cost = double(max_link_cost).  false: the link does not count (psr 0 or NaN, or a cost above the cap).
// The shortcut is E10's (errmodel_body): y2 < -1022 makes every term of the sum 0, so ber = 0 and psr = det_exp2(n * 0) = 1.
RM_HD bool route_link_cost(int kind, double us_per_bit, int64_t air_us, double noise_db, double max_cost, double rssi, uint32_t &cost)
{
    double psr = 1.0;
    if (kind == RM_EM_OQPSK_250K) {
        const double snr = rssi - noise_db;
        const double s = det_pow10(snr / 10.0);
        const double y2 = ((20.0 * s) * (1.0 / 2.0 - 1.0)) * 1.4426950408889634;
        if (!(y2 < -1022.0)) {
            const double ber = em_ber_oqpsk(s);
            psr = ber;
            if (ber == ber) psr = det_exp2((double(air_us) / us_per_bit) * det_log2(1.0 - ber));
        }
    }
    const double q = 128.0 / psr;
    const double c = floor(q + 0.5);
    if (!(psr > 0.0) || !(c <= max_cost)) return false;
    cost = uint32_t(c);
    return true;
}

// the measured-route query's entry cost: the rounded 128 * heard / delivered of one watched-link entry
// -- the text the kernels (rm_etx.hip) and rm_etx_link_cost / rm_etx_from_tables are both built from.  false: the entry is not
// usable or its cost is above the cap.  128 * H <= 2^47 and D >> 1 < 2^63: the sum cannot wrap.
// (etx_ratio: the quotient alone, for delivered >= 1 -- also what the neighbour tables judge a poor slot by, E22)
RM_HD uint64_t etx_ratio(uint64_t heard, uint64_t delivered)
{
    const uint64_t q = (128ull * heard + (delivered >> 1)) / delivered;
    return q < 128ull ? 128ull : q; // (a caller's table with delivered > heard)
}
RM_HD bool etx_entry_cost(uint32_t min_heard, uint32_t max_link_cost, uint64_t heard, uint64_t delivered, uint32_t &cost)
{
    const uint64_t least = min_heard > 1u ? uint64_t(min_heard) : 1ull;
    if (heard < least || heard > (1ull << 40) || delivered < 1ull) return false;
    const uint64_t q = etx_ratio(heard, delivered);
    if (q > uint64_t(max_link_cost)) return false;
    cost = uint32_t(q);
    return true;
}
// RM_ETX_BOTH: the product of the two directions' inbound costs, in units of 1/128
RM_HD uint64_t etx_combine(uint32_t c_in, uint32_t c_rev) { return (uint64_t(c_in) * uint64_t(c_rev) + 64ull) >> 7; }
// the order of two candidate links of one node: (c, p, k) ascending
RM_HD bool etx_precedes(uint32_t c, int32_t p, int k, uint32_t bc, int32_t bp, int bk)
{
    return c < bc || (c == bc && (p < bp || (p == bp && k < bk)));
}

// the link's uniform deviate: a hash of (seed, the frame's start, its source node, the receiver) and of nothing else -- not of
// packet numbers, ticks, slots or ranks, so a frame's verdict at a receiver is the same however the frame was evaluated
RM_HD double em_draw(uint64_t seed, int32_t src, int64_t start_us, int32_t dst)
{
    const uint64_t h1 = mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ uint64_t(start_us));
    const uint64_t h = mix64(h1 ^ ((uint64_t(uint32_t(src)) << 32) | uint64_t(uint32_t(dst))));
    return (double(h >> 12) + 0.5) * 0x1.0p-52;
}

// the receiver listening schedule: what a record may hold, and the listening rule -- the text the pass
// (rm_listen.hip) and rm_listen_at are both built from
RM_HD bool listen_valid(const rm_listen_schedule &s)
{
    if (s.period_us == 0) return s.on_us == 0 && s.phase_us == 0;
    return s.period_us > 0 && s.on_us >= 0 && s.on_us <= s.period_us && s.phase_us >= 0 && s.phase_us < s.period_us;
}

RM_HD bool listen_at(const rm_listen_schedule &s, int64_t t_us)
{
    if (s.period_us == 0) return true;
    const int64_t d = int64_t(uint64_t(t_us) - uint64_t(s.phase_us)); // (wraps)
    int64_t r = d % s.period_us;
    if (r < 0) r += s.period_us;
    return r < s.on_us;
}

// the watched-link statistics' fixed point: a dB value in 1/256 dB, rounded half up; 0 for NaN, an
// infinity and everything whose product would leave 64-bit range by far.  E-math: one multiplication, one addition, one floor --
// the text the pass (rm_linkstats.hip) and rm_linkstats_q8 are both built from
RM_HD int64_t linkstats_q8(double x)
{
    if (!(fabs(x) < 2147483648.0)) return 0;
    return int64_t(floor(x * 256.0 + 0.5));
}

// the forwarding queues' backoff: what the parameters may hold, and the backoff factor r of a node's
// `tries`-th failed attempt in a row at a frame that began at start_us -- the text the advance (rm_fwd.hip), rm_fwd_backoff and
// rm_fwd_validate are built from.  64-bit integers only.
RM_HD bool fwd_valid(const rm_fwd_params &p)
{
    const int q = p.queue_slots;
    if (!(q == 1 || q == 2 || q == 4 || q == 8 || q == 16)) return false;
    if (p.max_retries < 0 || p.max_retries > 15) return false;
    if (p.max_be < 0 || p.max_be > 8 || p.min_be < 0 || p.min_be > p.max_be) return false;
    if (p.max_hops < 1 || p.max_hops > 255) return false;
    return p.backoff_unit_us >= 0 && p.backoff_unit_us <= (int64_t(1) << 32) && p.reserved == 0;
}

RM_HD uint32_t fwd_backoff_factor(const uint64_t seed, const int32_t min_be, const int32_t max_be, const int32_t node, const int64_t start_us,
                                  const int32_t tries)
{
    const int64_t grown = int64_t(min_be) + int64_t(tries) - 1;
    const int be = int(grown < int64_t(max_be) ? grown : int64_t(max_be));
    if (be <= 0) return 0u;
    const uint64_t h1 = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ uint64_t(uint32_t(node))) ^ uint64_t(start_us));
    const uint64_t h2 = mix64(h1 ^ uint64_t(tries));
    return uint32_t(h2 >> (64 - be));
}

// the order of a queue's packets: the text the kernels' head search (rm_fwd.hip) and rm_fwd_queue_read are built from
RM_HD bool fwd_packet_order(const rm_fwd_packet &a, const rm_fwd_packet &b)
{
    if (a.enq_us != b.enq_us) return a.enq_us < b.enq_us;
    if (a.birth_us != b.birth_us) return a.birth_us < b.birth_us;
    if (a.origin != b.origin) return a.origin < b.origin;
    return a.hops < b.hops;
}

// the floods' Trickle schedule: what the parameters may hold, and interval m of a node that got the data
// at first_us -- where it starts and when the node fires in it; m >= max_intervals: done, both -1.  The text the kernels
// (rm_flood.hip), rm_flood_fire and rm_flood_validate are built from.  64-bit integers only.
RM_HD bool flood_valid(const rm_flood_params &p)
{
    if (p.imin_us < 2 || p.imin_us > (int64_t(1) << 32)) return false;
    if (p.doublings < 0 || p.doublings > 16 || p.max_intervals < 1 || p.max_intervals > 64) return false;
    return p.redundancy >= 0 && p.redundancy <= 255 && p.max_hops >= 1 && p.max_hops <= 65535;
}

RM_HD void flood_fire(const int64_t imin_us, const int32_t doublings, const int32_t max_intervals, const uint64_t seed, const int32_t node,
                      const int64_t first_us, const int32_t m, int64_t &start_us, int64_t &fire_us)
{
    if (m < 0 || m >= max_intervals) {
        start_us = fire_us = -1;
        return;
    }
    // the sum of I_i over i < m: the doubling ones are imin * (2^g - 1), g = min(m, D); the rest have the largest length
    const int g = m < doublings ? m : doublings;
    const int64_t len = imin_us << g; // (at most 2^48)
    const int64_t before = imin_us * ((int64_t(1) << g) - 1) + int64_t(m - g) * len;
    const uint64_t half = uint64_t(len >> 1);
    uint64_t h = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ uint64_t(uint32_t(node))) ^ uint64_t(first_us));
    h = mix64(h ^ uint64_t(m));
    start_us = first_us + before;
    fire_us = start_us + int64_t(half) + int64_t(uint64_t((static_cast<unsigned __int128>(h) * half) >> 64)); // (one text for host and device)
}

// the neighbour tables' rule: what the parameters may hold, the judgments of a slot, a bid's key and the
// choice of the slot a winning bid takes -- the text the kernels (rm_nbtable.hip), rm_nbtable_from_result, rm_nbtable_expire_tables
// and rm_nbtable_validate are built from.  Integers and one comparison of doubles only.
RM_HD bool nbt_valid(const rm_nbtable_params &p)
{
    if (!(fabs(p.admit_rssi_dbm) < INFINITY)) return false; // (NaN and the infinities)
    if (p.timeout_us < 0 || p.timeout_us > (int64_t(1) << 62) || p.min_heard > (1u << 31)) return false;
    if (p.evict_cost != 0u && p.evict_cost < 128u) return false;
    return (p.require_delivered == 0 || p.require_delivered == 1) && p.reserved == 0;
}
RM_HD bool nbt_in(int32_t n_nodes, int32_t j) { return j >= 0 && j < n_nodes; }
RM_HD bool nbt_empty(int32_t n_nodes, int32_t d, int32_t peer) { return !nbt_in(n_nodes, peer) || peer == d; }
RM_HD bool nbt_stale(int64_t timeout_us, int64_t t, int64_t last_start_us)
{
    if (timeout_us <= 0) return false;
    return last_start_us == INT64_MIN || (t >= timeout_us && last_start_us < t - timeout_us);
}
// c_in: UINT64_MAX with delivered == 0 (above every quotient)
RM_HD bool nbt_poor(const rm_nbtable_params &p, uint64_t heard, uint64_t delivered, uint64_t &c_in)
{
    if (p.evict_cost == 0u || heard < (p.min_heard > 1u ? uint64_t(p.min_heard) : 1ull)) return false;
    c_in = delivered == 0ull ? UINT64_MAX : etx_ratio(heard, delivered);
    return c_in > uint64_t(p.evict_cost);
}
// a bid's key: (qc, -s) in one word whose rest value 0 is below every bid
RM_HD uint64_t nbt_key(double rssi, int32_t s)
{
    int64_t qc = linkstats_q8(rssi);
    qc = qc < -(int64_t(1) << 30) ? -(int64_t(1) << 30) : (qc > (int64_t(1) << 30) ? (int64_t(1) << 30) : qc);
    return (uint64_t(qc + (int64_t(1) << 30) + 1) << 32) | uint64_t(0x7FFFFFFF - s);
}
RM_HD int32_t nbt_key_src(uint64_t key) { return int32_t(0x7FFFFFFF - int64_t(key & 0xFFFFFFFFull)); }
RM_HD bool nbt_bids(const rm_nbtable_params &p, double rssi, bool delivered)
{
    return rssi >= p.admit_rssi_dbm && (p.require_delivered == 0 || delivered);
}
// the slot of row d (peer[K], st[K], as at the start of the call) a winning bid takes: kind 0 an empty slot, 1 a stale one, 2 a
// poor one; -1: refused
RM_HD int nbt_settle(const rm_nbtable_params &p, int32_t n_nodes, int K, int32_t d, const int32_t *peer, const rm_link_stats *st, int64_t t,
                     int32_t pin, int &kind)
{
    kind = 0;
    for (int k = 0; k < K; ++k)
        if (nbt_empty(n_nodes, d, peer[k])) return k;
    const bool pinned = nbt_in(n_nodes, pin);
    int best = -1;
    kind = 1;
    for (int k = 0; k < K; ++k) {
        if ((pinned && peer[k] == pin) || !nbt_stale(p.timeout_us, t, st[k].last_start_us)) continue;
        if (best < 0 || st[k].last_start_us < st[best].last_start_us) best = k;
    }
    if (best >= 0) return best;
    uint64_t best_c = 0;
    kind = 2;
    for (int k = 0; k < K; ++k) {
        uint64_t c = 0;
        if ((pinned && peer[k] == pin) || !nbt_poor(p, st[k].heard, st[k].delivered, c)) continue;
        if (best < 0 || c > best_c) {
            best = k;
            best_c = c;
        }
    }
    return best;
}
RM_HD void nbt_clear(rm_link_stats &e)
{
    e.heard = e.delivered = 0;
    e.rssi_q8_sum = e.sinr_q8_sum = 0;
    e.first_start_us = INT64_MAX;
    e.last_start_us = INT64_MIN;
}

// the link estimator's rule: what the parameters may hold, the smoothing, a window's sample, the beacon
// step of one entry, the data step's judgment of one node and the published entry -- the text the kernel (rm_linkest.hip),
// rm_linkest_fold_tables and rm_linkest_validate are built from.  Unsigned integers only.
RM_HD bool lest_valid(const rm_linkest_params &p)
{
    if (p.beacon_window > (1u << 31) || p.data_window > (1u << 31)) return false;
    if (p.beacon_alpha_q8 > 255u || p.data_alpha_q8 > 255u) return false;
    return p.max_etx >= 128u && p.max_etx <= 65535u && p.reserved == 0u;
}
// alpha is the weight of the OLD estimate out of 256; 0: no estimate yet.  Between min(old, s) and max(old, s)
RM_HD uint32_t lest_ewma(uint32_t a, uint32_t old, uint32_t s)
{
    if (old == 0u) return s;
    return uint32_t((uint64_t(a) * old + uint64_t(256u - a) * s + 128ull) >> 8);
}
// a window of dn tries of which dd got through: 128 .. max_etx
RM_HD uint32_t lest_sample(uint32_t max_etx, uint64_t dn, uint64_t dd)
{
    if (dd == 0ull) return max_etx;
    const uint64_t q = etx_ratio(dn, dd);
    return q > uint64_t(max_etx) ? max_etx : uint32_t(q);
}
RM_HD void lest_restart(rm_linkest_entry &e, int32_t peer)
{
    e.base_heard = e.base_delivered = 0ull;
    e.etx = e.windows = e.data_windows = 0u;
    e.peer = peer;
}
enum { LEST_CLEARED = 1, LEST_RESTARTED = 2, LEST_SAMPLED = 4 };
// the beacon step of entry (j, k) whose input slot holds peer p with counters H, D: what happened, as LEST_* bits
RM_HD unsigned lest_beacon(const rm_linkest_params &p, int32_t n_nodes, int32_t j, int32_t peer, uint64_t H, uint64_t D, rm_linkest_entry &e)
{
    if (nbt_empty(n_nodes, j, peer)) {
        const unsigned did = e.peer != -1 ? unsigned(LEST_CLEARED) : 0u;
        lest_restart(e, -1);
        return did;
    }
    unsigned did = 0u;
    if (peer != e.peer || H < e.base_heard || D < e.base_delivered) {
        lest_restart(e, peer);
        did = LEST_RESTARTED;
    }
    const uint64_t dH = H - e.base_heard, dD = D - e.base_delivered;
    if (p.beacon_window > 0u && dH >= uint64_t(p.beacon_window)) {
        e.etx = lest_ewma(p.beacon_alpha_q8, e.etx, lest_sample(p.max_etx, dH, dD));
        e.windows += 1u;
        e.base_heard = H;
        e.base_delivered = D;
        did |= LEST_SAMPLED;
    }
    return did;
}
// the data step's judgment of node j whose forwarding row says next hop w, T = acked + failed, A = acked: true when a sample of
// (dT, dA) toward w is due (the bases are moved either way)
RM_HD bool lest_data(const rm_linkest_params &p, int32_t n_nodes, int32_t j, int32_t w, uint64_t T, uint64_t A, rm_linkest_node &nd, uint64_t &dT,
                     uint64_t &dA)
{
    if (w != nd.base_next || T < nd.base_tx || A < nd.base_ack) {
        nd.base_next = w;
        nd.base_tx = T;
        nd.base_ack = A;
        return false;
    }
    if (!nbt_in(n_nodes, w) || w == j || T - nd.base_tx < uint64_t(p.data_window)) return false;
    dT = T - nd.base_tx;
    dA = A - nd.base_ack;
    nd.base_tx = T;
    nd.base_ack = A;
    return true;
}
RM_HD void lest_data_sample(const rm_linkest_params &p, uint64_t dT, uint64_t dA, rm_linkest_entry &e)
{
    e.etx = lest_ewma(p.data_alpha_q8, e.etx, lest_sample(p.max_etx, dT, dA));
    e.data_windows += 1u;
}
// the published entry: c_in of the measured-route query is exactly etx
RM_HD void lest_publish(uint32_t etx, rm_link_stats &s)
{
    nbt_clear(s);
    if (etx != 0u) {
        s.heard = uint64_t(etx);
        s.delivered = 128ull;
    }
}

// the traffic schedule: what a record may hold, a packet's due time, and the number of a node's packets
// due before a time -- the text the generator (rm_traffic.hip), rm_traffic_due and rm_traffic_validate are all built from.
// 64-bit integers only.
constexpr int64_t kTrafficMaxPeriod = int64_t(1) << 40;
constexpr int64_t kTrafficMaxTime = int64_t(1) << 62;

RM_HD bool traffic_valid(const rm_traffic_schedule &s)
{
    if (s.reserved != 0) return false;
    if (s.period_us == 0) return s.phase_us == 0 && s.jitter_us == 0;
    return s.period_us >= 1 && s.period_us <= kTrafficMaxPeriod && s.phase_us >= 0 && s.phase_us < s.period_us && s.jitter_us >= 0 &&
           s.jitter_us <= s.period_us;
}

// j(i, k): 0 without jitter, otherwise the high half of h * jitter_us, so 0 <= j < jitter_us
RM_HD int64_t traffic_jitter(const rm_traffic_schedule &s, uint64_t seed, int32_t node, int64_t k)
{
    if (s.jitter_us == 0) return 0;
    const uint64_t h = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ uint64_t(uint32_t(node))) ^ uint64_t(k));
#if defined(__HIP_DEVICE_COMPILE__)
    return int64_t(__umul64hi(h, uint64_t(s.jitter_us)));
#else
    return int64_t(uint64_t((static_cast<unsigned __int128>(h) * uint64_t(s.jitter_us)) >> 64));
#endif
}

// due(i, k) of a valid record with period_us > 0, for k >= 0 with k * period_us <= 2^62 (no overflow below that)
RM_HD int64_t traffic_due(const rm_traffic_schedule &s, uint64_t seed, int32_t node, int64_t k)
{
    return s.phase_us + k * s.period_us + traffic_jitter(s, seed, node, k);
}

// The number of the node's packets with due < t (0 <= t <= 2^62; period_us > 0), which is also the number of the first packet
// due at t or later, because due grows strictly with k.  With e = the last packet whose jitter interval BEGINS before t, every
// packet before e is due before t (its interval ends before e's begins: jitter <= period), every one after e is not, and e
// itself needs its hash only when its interval reaches t.  n is a lower bound of the answer the caller knows (0: nothing is
// known -- the answer of an earlier time is one): up to one period behind packet n's interval no division is needed.
RM_HD int64_t traffic_before(const rm_traffic_schedule &s, uint64_t seed, int32_t node, int64_t t, int64_t n)
{
    const int64_t period = s.period_us;
    const int64_t base_n = s.phase_us + n * period;
    if (t <= base_n) return n;
    const int64_t e = (t - base_n <= period) ? n : (t - 1 - s.phase_us) / period;
    const int64_t base = s.phase_us + e * period;
    if (base + s.jitter_us <= t) return e + 1; // (the whole interval, base .. base + jitter - 1, lies before t; jitter 0: base < t)
    return e + (base + traffic_jitter(s, seed, node, e) < t ? 1 : 0);
}

// Position.getDistance, Position.java:56-64: this = transmitter, p2 = receiver;
// (dx*dx + dy*dy) + dz*dz, then a correctly rounded square root.
RM_HD double ref_distance(double ax, double ay, double az, double bx, double by, double bz)
{
    double dx = ax - bx;
    double dy = ay - by;
    double dz = az - bz;
    dx = dx * dx;
    dy = dy * dy;
    dz = dz * dz;
    return sqrt(dx + dy + dz);
}

RM_HD double logdist_rssi(const ModelDev &m, const rm_tx_record &tx, double rx, double ry, double rz, int j)
{
    const double d = ref_distance(tx.x, tx.y, tx.z, rx, ry, rz);
    const double dd = (d > m.ld_d0) ? d : m.ld_d0;
    const double t1 = tx.txpower - m.ld_pl0;
    const double t2 = 10.0 * m.ld_exp;
    const double l = det_log10(dd / m.ld_d0);
    double rssi = t1 - t2 * l;
    if (m.ld_sigma > 0.0) {
        rssi = rssi - m.ld_sigma * shadow_gauss(m.ld_seed_mixed, m.ld_clip, uint32_t(tx.src), uint32_t(j));
    }
    return rssi;
}

// ---- Q80 fixed point (exact, order-independent interference sums) ------------------------
struct U128 {
    uint64_t lo, hi;
};

RM_HD U128 u128_add(U128 a, U128 b)
{
    U128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1u : 0u);
    return r;
}

RM_HD U128 u128_sub(U128 a, U128 b) // a >= b
{
    U128 r;
    r.lo = a.lo - b.lo;
    r.hi = a.hi - b.hi - (a.lo < b.lo ? 1u : 0u);
    return r;
}

RM_HD U128 q80_from_double(double lin)
{
    U128 r = {0, 0};
    if (!(lin > 0.0)) return r;
    const uint64_t bits = f2u(lin);
    const int ex = int((bits >> 52) & 0x7FFu);
    if (ex == 0x7FF) {
        r.lo = ~0ull;
        r.hi = 0x7FFFFFFFFFFFFFFFull;
        return r;
    }
    if (ex == 0) return r;
    const uint64_t man = (bits & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull;
    const int shift = ex - 1075 + 80;
    if (shift >= 0) {
        if (shift > 74) {
            r.lo = ~0ull;
            r.hi = 0x7FFFFFFFFFFFFFFFull;
            return r;
        }
        if (shift >= 64) {
            r.hi = man << (shift - 64);
        } else if (shift == 0) {
            r.lo = man;
        } else {
            r.lo = man << shift;
            r.hi = man >> (64 - shift);
        }
        return r;
    }
    if (-shift >= 64) return r;
    r.lo = man >> (-shift);
    return r;
}

RM_HD int clz64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

RM_HD double q80_to_double(U128 q)
{
    if (q.hi == 0 && q.lo == 0) return 0.0;
    const int top = q.hi ? 127 - clz64(q.hi) : 63 - clz64(q.lo);
    uint64_t keep;
    int drop = 0;
    if (top <= 52) {
        keep = q.lo;
    } else {
        drop = top - 52;
        // keep = q >> drop ; rem = q & ((1<<drop)-1)
        uint64_t rem_hi, rem_lo, half_hi, half_lo;
        if (drop >= 64) {
            keep = q.hi >> (drop - 64);
            rem_hi = (drop == 64) ? 0 : (q.hi & ((1ull << (drop - 64)) - 1));
            rem_lo = q.lo;
            half_hi = (drop == 64) ? 0 : (1ull << (drop - 65));
            half_lo = (drop == 64) ? (1ull << 63) : 0;
        } else {
            keep = (q.lo >> drop) | (q.hi << (64 - drop));
            rem_hi = 0;
            rem_lo = q.lo & ((1ull << drop) - 1);
            half_hi = 0;
            half_lo = 1ull << (drop - 1);
        }
        const bool gt = (rem_hi > half_hi) || (rem_hi == half_hi && rem_lo > half_lo);
        const bool eq = (rem_hi == half_hi) && (rem_lo == half_lo);
        if (gt || (eq && (keep & 1ull))) keep += 1;
    }
    // keep * 2^(drop-80): both factors exact
    const double scale = u2f(uint64_t(drop - 80 + 1023) << 52);
    return double(keep) * scale;
}

// ---- java.util.Random (Java SE specification) ----------------------------------------------
constexpr uint64_t kLcgA = 0x5DEECE66Dull;
constexpr uint64_t kLcgC = 0xBull;
constexpr uint64_t kLcgMask = (1ull << 48) - 1;

// affine map of `steps` LCG steps: s -> A*s + C (mod 2^48)
RM_HD void lcg_jump_map(uint64_t steps, uint64_t &A, uint64_t &C)
{
    uint64_t a = kLcgA, c = kLcgC;
    uint64_t accA = 1, accC = 0;
    while (steps) {
        if (steps & 1ull) {
            accA = (accA * a) & kLcgMask;
            accC = (accC * a + c) & kLcgMask;
        }
        c = ((a + 1) * c) & kLcgMask;
        a = (a * a) & kLcgMask;
        steps >>= 1;
    }
    A = accA;
    C = accC;
}


RM_HD double lcg_next_double(uint64_t &s)
{
    s = (s * kLcgA + kLcgC) & kLcgMask;
    const int64_t hi = int64_t(s >> 22); // next(26)
    s = (s * kLcgA + kLcgC) & kLcgMask;
    const int64_t lo = int64_t(s >> 21); // next(27)
    return double((hi << 27) + lo) * 0x1.0p-53;
}

} // namespace rm
