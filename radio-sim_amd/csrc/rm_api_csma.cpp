// rm_api_csma.cpp -- C ABI: the CSMA-CA gated batch (rm_batch_run_sources_csma*, rm_csma_schedule; rm_csma.hip)
// and its carry (rm_batch_run_sources_csma_carry*, rm_csma_schedule_carry, rm_csma_carry_collect*; E9).
//
// A deferred candidate backs off and senses again in a later tick of the same batch.  The backoff draw is a hash of the packet and the
// attempt number, so the host lays out every attempt of every packet before anything is launched (csma_schedule): attempts are extra
// slots of their ticks' lists.  The gate then is the gated batch's (rm_api_cca.cpp) over those expanded lists, with one state per
// packet in the serial pass, and the unchanged batch runs over the gated expanded lists.
// A carried packet (E9) is one more packet, n_pkt + its place in the carry list, whose chain begins at a later attempt in a tick
// the caller names: the batch without a carry is the batch with an empty one.
#include "rm_host.hpp"

using namespace rmh;

namespace {

struct Schedule {
    std::vector<int32_t> n_exp, first, own_first, origin, next_tick; // per tick (first / own_first: n_ticks + 1), per slot
    std::vector<uint8_t> attempt;
    int64_t total = 0;
};

int csma_params_check(const rm_csma_params *p)
{
    if (!p) return fail(RM_ERR_INVALID, "rm_csma_params is NULL");
    if (p->max_backoffs < 0 || p->max_backoffs > 5) return fail(RM_ERR_INVALID, "max_backoffs outside 0 .. 5");
    if (p->max_be < 0 || p->max_be > 8 || p->min_be < 0 || p->min_be > p->max_be) return fail(RM_ERR_INVALID, "0 <= min_be <= max_be <= 8 does not hold");
    if (p->reserved != 0) return fail(RM_ERR_INVALID, "rm_csma_params.reserved has to be 0");
    return RM_OK;
}

// the tick of attempt a + 1 of the packet in slot k of a tick whose sample time hashed to h1, given attempt a's tick
int64_t csma_next_tick(const rm_csma_params &p, uint64_t h1, int32_t k, int a, int64_t tick)
{
    const int be = std::min(p.min_be + a, p.max_be);
    const uint64_t h2 = rm::host_mix64(h1 ^ ((uint64_t(uint32_t(k)) << 8) | uint64_t(a)));
    return tick + 1 + (be == 0 ? 0 : int64_t(h2 >> (64 - be)));
}

// counts only (fill = false: n_exp, first, own_first, total), or the slots too.  The carried packets are walked first, in list order,
// then the packets in (origin tick, origin slot) order, and a packet has at most one attempt per tick: appending to the ticks' cursors
// leaves every tick's list in the order of the contract -- own entries, carried attempts, own retries.  attempt[] carries rm::kCsFirst
// on the first slot of a packet's chain in this batch (an own packet's attempt 0, a carried packet's attempt carry[c].attempt).
void csma_schedule(const rm_csma_params &p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us, const rm_csma_carry *carry,
                   int32_t n_carry, Schedule &s, bool fill)
{
    const uint64_t seed_mixed = rm::host_mix64(p.seed + 0x9E3779B97F4A7C15ull);
    s.n_exp.assign(n_src, n_src + n_ticks);
    s.own_first.assign(size_t(n_ticks) + 1, 0);
    for (int b = 0; b < n_ticks; ++b) s.own_first[size_t(b) + 1] = s.own_first[size_t(b)] + n_src[b];
    const int32_t n_pkt = s.own_first[size_t(n_ticks)];
    for (int pass = 0; pass < (fill ? 2 : 1); ++pass) {
        std::vector<int32_t> cursor;
        if (pass == 1) {
            s.origin.resize(size_t(s.total));
            s.next_tick.resize(size_t(s.total));
            s.attempt.resize(size_t(s.total));
            cursor.resize(size_t(n_ticks));
            for (int b = 0; b < n_ticks; ++b) cursor[size_t(b)] = s.first[size_t(b)] + n_src[b];
        }
        // packet o's chain from attempt a0 in tick `tick` on; slot: where that attempt sits (pass 1)
        auto chain = [&](uint64_t h1, int32_t k, int a0, int64_t tick, int32_t o, int32_t slot) {
            for (int a = a0; a <= p.max_backoffs; ++a) {
                const int64_t next = a < p.max_backoffs ? csma_next_tick(p, h1, k, a, tick) : -1;
                if (pass == 1) {
                    s.origin[size_t(slot)] = o;
                    s.attempt[size_t(slot)] = uint8_t(a | (a == a0 ? rm::kCsFirst : 0));
                    s.next_tick[size_t(slot)] = int32_t(next);
                }
                if (next < 0 || next >= n_ticks) break;
                tick = next;
                if (pass == 0) ++s.n_exp[size_t(tick)];
                else slot = cursor[size_t(tick)]++;
            }
        };
        for (int32_t c = 0; c < n_carry; ++c) {
            const rm_csma_carry &r = carry[c];
            if (r.tick >= n_ticks) continue; // (no slot in this batch: still pending)
            int32_t slot = 0;
            if (pass == 0) ++s.n_exp[size_t(r.tick)];
            else slot = cursor[size_t(r.tick)]++;
            chain(rm::host_mix64(seed_mixed ^ uint64_t(r.origin_cca_time_us)), r.origin_slot, r.attempt, r.tick, n_pkt + c, slot);
        }
        for (int b = 0; b < n_ticks; ++b) {
            const uint64_t h1 = rm::host_mix64(seed_mixed ^ uint64_t(cca_time_us[b]));
            for (int32_t k = 0; k < n_src[b]; ++k) chain(h1, k, 0, b, s.own_first[size_t(b)] + k, pass == 1 ? s.first[size_t(b)] + k : 0);
        }
        if (pass == 0) {
            s.first.assign(size_t(n_ticks) + 1, 0);
            int64_t at = 0;
            for (int b = 0; b < n_ticks; ++b) {
                s.first[size_t(b)] = int32_t(at);
                at += s.n_exp[size_t(b)];
            }
            s.first[size_t(n_ticks)] = int32_t(at);
            s.total = at;
        }
    }
}

// a packet contributes at most 1 + max_backoffs <= 6 slots: with at most 2^27 packets (carried ones included) the slot count stays
// below the 2^30 the pair list's slot field holds
constexpr size_t kCsmaMaxPackets = size_t(1) << 27;

// the carry list as such (p: checked)
int csma_carry_check(const rm_csma_params &p, const rm_csma_carry *carry, int32_t n_carry, int32_t n_nodes)
{
    if (n_carry < 0 || (n_carry > 0 && !carry)) return fail(RM_ERR_INVALID, "bad carry list");
    for (int32_t c = 0; c < n_carry; ++c) {
        const rm_csma_carry &r = carry[c];
        if (n_nodes >= 0 && (r.node < 0 || r.node >= n_nodes)) return fail(RM_ERR_INVALID, "a carried packet's node is outside 0 .. n_nodes-1");
        if (r.attempt < 1 || r.attempt > p.max_backoffs) return fail(RM_ERR_INVALID, "a carried packet's attempt is outside 1 .. max_backoffs");
        if (r.tick < 0 || r.origin_slot < 0) return fail(RM_ERR_INVALID, "a carried packet's tick or origin_slot is negative");
    }
    return RM_OK;
}

// what both forms refuse, before anything is launched and with nothing changed; leaves the schedule in `s`
int csma_check(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src, const int32_t *n_src,
               const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us, const rm_csma_params *p, const rm_csma_carry *carry,
               int32_t n_carry, Schedule &s)
{
    RM_TRY(cca_batch_check_lists(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us));
    RM_TRY(csma_params_check(p));
    RM_TRY(csma_carry_check(*p, carry, n_carry, c->n));
    size_t n_pkt = size_t(n_carry);
    for (int b = 0; b < n_ticks; ++b) n_pkt += size_t(n_src[b]);
    if (n_pkt > kCsmaMaxPackets) return fail(RM_ERR_CAPACITY, "more than 2^27 packets in one CSMA-CA gated batch");
    csma_schedule(*p, n_ticks, n_src, cca_time_us, carry, n_carry, s, true);
    return cca_batch_check_ticks(c, n_ticks, t_begin_us, s.n_exp.data(), start_us, air_us, cca_time_us);
}

// src[b], out's and carried_out's pointers: device-visible memory
int csma_batch(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src, const int32_t *n_src,
               const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us, double cca_threshold, const Schedule &s,
               const rm_csma_result *out, int32_t *n_exp, const rm_csma_carry *carry, int32_t n_carry, const rm_csma_result *carried_out)
{
    RM_HIP(hipSetDevice(c->device));
    const size_t n_slots = size_t(s.total), n_pkt = size_t(s.own_first[size_t(n_ticks)]);
    const size_t carry_bytes = size_t(n_carry) * sizeof(rm_csma_carry);
    rm_context::Energy &e = c->ed;
    rm_context::Energy::Batch &k = e.cb;
    rm_context::Energy::Csma &q = e.cs;
    static thread_local std::vector<const int32_t *> gated_v;
    gated_v.assign(size_t(n_ticks), nullptr);
    if (n_slots > 0) {
        // the window as the batch will find it (batch_run does both again and finds nothing left to do)
        RM_TRY(air_window_expire(c, t_begin_us[0]));
        RM_TRY(air_window_reserve(c, n_slots));
        // the schedule goes up through the pinned block that carries the tick descriptors: origin, next tick, first packet per tick, attempt
        const size_t off_next = pad64(n_slots * 4), off_own = off_next + pad64(n_slots * 4), off_att = off_own + pad64((size_t(n_ticks) + 1) * 4);
        const size_t off_carry = off_att + pad64(n_slots);
        const size_t bytes = off_carry + pad64(carry_bytes);
        rm::CsmaDev cs{};
        bool grid = false;
        rm::CcaTick *h_ticks = nullptr;
        char *h_up = nullptr;
        RM_TRY(cca_batch_dev(c, n_slots, n_ticks, src, s.n_exp.data(), start_us, air_us, cca_time_us, bytes, &cs.cb, &grid, &h_ticks, gated_v.data(), &h_up));
        uint32_t *const h_info = cs.cb.h_info;
        std::memcpy(h_up, s.origin.data(), n_slots * 4);
        std::memcpy(h_up + off_next, s.next_tick.data(), n_slots * 4);
        std::memcpy(h_up + off_own, s.own_first.data(), (size_t(n_ticks) + 1) * 4);
        std::memcpy(h_up + off_att, s.attempt.data(), n_slots);
        if (n_carry > 0) std::memcpy(h_up + off_carry, carry, carry_bytes);
        RM_HIP(q.sched.ensure(bytes));
        RM_HIP(q.state.ensure(std::max<size_t>(n_pkt + size_t(n_carry), 1)));
        RM_HIP(q.tentative.ensure(n_slots));
        RM_HIP(q.slot_flags.ensure(n_slots));
        RM_HIP(hipMemcpyAsync(q.sched.p, h_up, bytes, hipMemcpyHostToDevice, c->stream));
        cs.origin = reinterpret_cast<const int32_t *>(q.sched.p);
        cs.next_tick = reinterpret_cast<const int32_t *>(q.sched.p + off_next);
        cs.own_first = reinterpret_cast<const int32_t *>(q.sched.p + off_own);
        cs.attempt = reinterpret_cast<const uint8_t *>(q.sched.p + off_att);
        cs.n_pkt = int(n_pkt);
        cs.carry = reinterpret_cast<const rm_csma_carry *>(q.sched.p + off_carry);
        cs.n_carry = n_carry;
        if (carried_out) cs.carried = *carried_out;
        cs.state = q.state.p;
        cs.tentative = q.tentative.p;
        cs.slot_flags = q.slot_flags.p;
        if (out) cs.out = *out;
        rm::ModelDev m = model_dev(c);
        if (c->f32_slack > 0.05) m.shadow_tbl = nullptr; // (as the query: the link-hash table goes with the fp32 filter of a small frame)
        {
            CallProbe probe(c); // (rm_profile_kernels names the kernels that ran)
            sample_stage(probe.smp, RM_STAGE_SINR);
            h_info[0] = 0u;
            RM_HIP(rm::launch_csma_count(c->stream, nodes_dev(c), m, cs, h_ticks, k.ticks.p, grid));
            // the one place where the host has to know a number of the device's: the pairs of all slots, counted, not guessed
            RM_HIP(hipStreamSynchronize(c->stream));
            if (h_info[1] != 0u) return fail(RM_ERR_HIP, "internal: a candidate's pairs outgrew their counted segment in an earlier gated batch");
            if (h_info[0] == 0xFFFFFFFFu) return fail(RM_ERR_CAPACITY, "more than 2^32 (slot, frame) pairs in one CSMA-CA gated batch: use smaller batches");
            const size_t n_pairs = std::max<size_t>(h_info[0], 1);
            RM_HIP(k.pair_slot.ensure(n_pairs));
            RM_HIP(k.pair_term.ensure(n_pairs));
            cs.cb.pair_slot = k.pair_slot.p;
            cs.cb.pair_term = k.pair_term.p;
            RM_HIP(rm::launch_csma_resolve(c->stream, nodes_dev(c), m, cs, grid, cca_threshold, e.gated.p));
        }
    }
    if (n_slots == 0 && n_carry > 0) {
        // carried packets, none with a slot in this batch: their entries, nothing else (the records go up through the pinned block)
        rm::CcaTick *h_ticks = nullptr;
        uint32_t *h_info = nullptr;
        char *h_up = nullptr;
        RM_TRY(cca_desc_block(c, pad64(carry_bytes), &h_ticks, &h_info, &h_up));
        std::memcpy(h_up, carry, carry_bytes);
        RM_HIP(q.sched.ensure(pad64(carry_bytes)));
        RM_HIP(q.state.ensure(n_pkt + size_t(n_carry)));
        RM_HIP(hipMemcpyAsync(q.sched.p, h_up, carry_bytes, hipMemcpyHostToDevice, c->stream));
        rm::CsmaDev cs{};
        cs.cb.n_ticks = n_ticks;
        cs.n_pkt = int(n_pkt);
        cs.carry = reinterpret_cast<const rm_csma_carry *>(q.sched.p);
        cs.n_carry = n_carry;
        cs.state = q.state.p;
        if (carried_out) cs.carried = *carried_out;
        RM_HIP(rm::launch_csma_slotless(c->stream, cs));
        // (the pinned block is free again once the copy has landed: the next gated batch writes it before it launches anything)
        RM_HIP(hipStreamSynchronize(c->stream));
    }
    if (n_exp) std::memcpy(n_exp, s.n_exp.data(), size_t(n_ticks) * 4);
    // the unchanged batch over the gated expanded lists (a batch without packets keeps its NULL lists)
    const int rc = batch_run(c, n_ticks, t_begin_us, t_end_us, gated_v.data(), nullptr, s.n_exp.data(), start_us, air_us);
    ev_batch_ran(c, rc, n_ticks, true);
    return rc;
}

// what both collects refuse; *n_pkt: the own packets
int collect_check(int32_t n_ticks, const int32_t *const *src, const int32_t *n_src, const int64_t *cca_time_us, const rm_csma_carry *carry,
                  int32_t n_carry, const rm_csma_result *out, const rm_csma_result *carried_out, const rm_csma_carry *carry_out, int64_t cap,
                  size_t *n_pkt)
{
    if (n_ticks < 1 || n_ticks > RM_MAX_BATCH || !src || !n_src || !cca_time_us || n_carry < 0 || (n_carry > 0 && !carry) || cap < 0 ||
        (cap > 0 && !carry_out))
        return fail(RM_ERR_INVALID, "bad arguments");
    size_t n = 0;
    for (int b = 0; b < n_ticks; ++b) {
        if (n_src[b] < 0 || (n_src[b] > 0 && !src[b])) return fail(RM_ERR_INVALID, "bad arguments");
        n += size_t(n_src[b]);
    }
    if (n + size_t(n_carry) > kCsmaMaxPackets) return fail(RM_ERR_CAPACITY, "more than 2^27 packets in one CSMA-CA gated batch");
    if (n > 0 && !(out && out->status && out->attempts && out->tick))
        return fail(RM_ERR_INVALID, "the carry-out needs the packets' status, attempts and tick");
    if (n_carry > 0 && !(carried_out && carried_out->status && carried_out->attempts && carried_out->tick))
        return fail(RM_ERR_INVALID, "the carry-out needs the carried packets' status, attempts and tick");
    *n_pkt = n;
    return RM_OK;
}

} // namespace

extern "C" {

void rm_csma_defaults(rm_csma_params *p)
{
    if (!p) return;
    p->max_backoffs = 4;
    p->min_be = 3;
    p->max_be = 5;
    p->reserved = 0;
    p->seed = 0;
}

int rm_csma_schedule_carry(const rm_csma_params *p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us, const rm_csma_carry *carry,
                           int32_t n_carry, int32_t *n_exp, int32_t *origin, uint8_t *attempt, int64_t cap, int64_t *total)
{
    RM_TRY(csma_params_check(p));
    if (n_ticks < 1 || n_ticks > RM_MAX_BATCH || !n_src || !cca_time_us || cap < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(csma_carry_check(*p, carry, n_carry, -1)); // (no table here: any node)
    size_t n_pkt = size_t(n_carry);
    for (int b = 0; b < n_ticks; ++b) {
        if (n_src[b] < 0) return fail(RM_ERR_INVALID, "bad arguments");
        n_pkt += size_t(n_src[b]);
    }
    if (n_pkt > kCsmaMaxPackets) return fail(RM_ERR_CAPACITY, "more than 2^27 packets in one CSMA-CA gated batch");
    static thread_local Schedule s;
    const bool fill = origin != nullptr || attempt != nullptr;
    csma_schedule(*p, n_ticks, n_src, cca_time_us, carry, n_carry, s, false);
    if (n_exp) std::memcpy(n_exp, s.n_exp.data(), size_t(n_ticks) * 4);
    if (total) *total = s.total;
    if (!fill) return RM_OK;
    if (cap < s.total) return fail(RM_ERR_CAPACITY, "origin / attempt have room for fewer entries than the expanded lists hold");
    csma_schedule(*p, n_ticks, n_src, cca_time_us, carry, n_carry, s, true);
    if (origin && s.total > 0) std::memcpy(origin, s.origin.data(), size_t(s.total) * 4);
    if (attempt)
        for (int64_t i = 0; i < s.total; ++i) attempt[i] = uint8_t(s.attempt[size_t(i)] & ~rm::kCsFirst);
    return RM_OK;
}

int rm_csma_schedule(const rm_csma_params *p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us, int32_t *n_exp, int32_t *origin,
                     uint8_t *attempt, int64_t cap, int64_t *total)
{
    return rm_csma_schedule_carry(p, n_ticks, n_src, cca_time_us, nullptr, 0, n_exp, origin, attempt, cap, total);
}

int rm_batch_run_sources_csma_carry_device(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                           const int32_t *const *dev_src, const int32_t *n_src, const int64_t *start_us, const int64_t *air_us,
                                           const int64_t *cca_time_us, double cca_threshold_dbm, const rm_csma_params *p,
                                           const rm_csma_result *dev_out, int32_t *n_exp, const rm_csma_carry *carry, int32_t n_carry,
                                           const rm_csma_result *dev_carried_out)
{
    static thread_local Schedule s;
    RM_TRY(csma_check(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us, p, carry, n_carry, s));
    return csma_batch(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, s, dev_out, n_exp, carry,
                      n_carry, dev_carried_out);
}

int rm_batch_run_sources_csma_device(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *dev_src,
                                     const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                                     double cca_threshold_dbm, const rm_csma_params *p, const rm_csma_result *dev_out, int32_t *n_exp)
{
    return rm_batch_run_sources_csma_carry_device(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us,
                                                  cca_threshold_dbm, p, dev_out, n_exp, nullptr, 0, nullptr);
}

int rm_batch_run_sources_csma_carry(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                                    const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                                    double cca_threshold_dbm, const rm_csma_params *p, const rm_csma_result *out, int32_t *n_exp,
                                    const rm_csma_carry *carry, int32_t n_carry, const rm_csma_result *carried_out)
{
    static thread_local Schedule s;
    RM_TRY(csma_check(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us, p, carry, n_carry, s));
    size_t total = 0;
    for (int b = 0; b < n_ticks; ++b) {
        for (int32_t k = 0; k < n_src[b]; ++k)
            if (src[b][k] < -1 || src[b][k] >= c->n) return fail(RM_ERR_INVALID, "source index out of range (-1 .. n_nodes-1)");
        total += size_t(n_src[b]);
    }
    RM_HIP(hipSetDevice(c->device));
    static thread_local std::vector<const int32_t *> lists;
    lists.assign(size_t(n_ticks), nullptr);
    rm_context::Energy::Csma &q = c->ed.cs;
    rm_csma_result dev{}, dev_c{};
    if (total > 0) {
        double *h_energy = nullptr;
        int32_t *h_src = nullptr;
        uint8_t *h_flags = nullptr;
        RM_TRY(energy_host_block(c, int32_t(total), &h_energy, &h_src, &h_flags)); // (the lists go in through the query's pinned block)
        size_t at = 0;
        for (int b = 0; b < n_ticks; ++b) {
            if (n_src[b] > 0) std::memcpy(h_src + at, src[b], size_t(n_src[b]) * 4);
            lists[size_t(b)] = h_src + at;
            at += size_t(n_src[b]);
        }
        RM_HIP(q.o_status.ensure(total));
        RM_HIP(q.o_attempts.ensure(total));
        RM_HIP(q.o_flags.ensure(total));
        RM_HIP(q.o_tick.ensure(total));
        RM_HIP(q.o_pkt.ensure(total));
        RM_HIP(q.o_energy.ensure(total));
        dev = rm_csma_result{q.o_status.p, q.o_attempts.p, q.o_tick.p, q.o_pkt.p, q.o_flags.p, q.o_energy.p};
    }
    const size_t nc = size_t(n_carry);
    if (nc > 0) {
        RM_HIP(q.c_status.ensure(nc));
        RM_HIP(q.c_attempts.ensure(nc));
        RM_HIP(q.c_flags.ensure(nc));
        RM_HIP(q.c_tick.ensure(nc));
        RM_HIP(q.c_pkt.ensure(nc));
        RM_HIP(q.c_energy.ensure(nc));
        dev_c = rm_csma_result{q.c_status.p, q.c_attempts.p, q.c_tick.p, q.c_pkt.p, q.c_flags.p, q.c_energy.p};
    }
    RM_TRY(csma_batch(c, n_ticks, t_begin_us, t_end_us, lists.data(), n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, s, &dev, n_exp, carry,
                      n_carry, &dev_c));
    RM_HIP(hipStreamSynchronize(c->stream));
    const struct { const rm_csma_result *to, *from; size_t n; } tables[2] = {{out, &dev, total}, {carried_out, &dev_c, nc}};
    for (const auto &t : tables) {
        if (t.n == 0 || !t.to) continue;
        if (t.to->status) RM_HIP(hipMemcpy(t.to->status, t.from->status, t.n, hipMemcpyDeviceToHost));
        if (t.to->attempts) RM_HIP(hipMemcpy(t.to->attempts, t.from->attempts, t.n, hipMemcpyDeviceToHost));
        if (t.to->tick) RM_HIP(hipMemcpy(t.to->tick, t.from->tick, t.n * 4, hipMemcpyDeviceToHost));
        if (t.to->pkt) RM_HIP(hipMemcpy(t.to->pkt, t.from->pkt, t.n * 4, hipMemcpyDeviceToHost));
        if (t.to->flags) RM_HIP(hipMemcpy(t.to->flags, t.from->flags, t.n, hipMemcpyDeviceToHost));
        if (t.to->energy_dbm) RM_HIP(hipMemcpy(t.to->energy_dbm, t.from->energy_dbm, t.n * 8, hipMemcpyDeviceToHost));
    }
    return RM_OK;
}

int rm_batch_run_sources_csma(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                              const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                              double cca_threshold_dbm, const rm_csma_params *p, const rm_csma_result *out, int32_t *n_exp)
{
    return rm_batch_run_sources_csma_carry(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, p, out,
                                           n_exp, nullptr, 0, nullptr);
}

int rm_csma_carry_collect(int32_t n_ticks, const int32_t *const *src, const int32_t *n_src, const int64_t *cca_time_us, const rm_csma_carry *carry,
                          int32_t n_carry, const rm_csma_result *out, const rm_csma_result *carried_out, rm_csma_carry *carry_out, int64_t cap,
                          int64_t *count)
{
    size_t n_pkt = 0;
    RM_TRY(collect_check(n_ticks, src, n_src, cca_time_us, carry, n_carry, out, carried_out, carry_out, cap, &n_pkt));
    int64_t n = 0;
    auto put = [&](const rm_csma_carry &r) {
        if (n < cap) carry_out[n] = r;
        ++n;
    };
    for (int32_t c = 0; c < n_carry; ++c)
        if (carried_out->status[c] == RM_CSMA_PENDING)
            put(rm_csma_carry{carry[c].origin_cca_time_us, carry[c].origin_slot, carry[c].node, carried_out->tick[c] - n_ticks, carried_out->attempts[c]});
    size_t o = 0;
    for (int b = 0; b < n_ticks; ++b)
        for (int32_t k = 0; k < n_src[b]; ++k, ++o)
            if (out->status[o] == RM_CSMA_PENDING) put(rm_csma_carry{cca_time_us[b], k, src[b][k], out->tick[o] - n_ticks, out->attempts[o]});
    if (count) *count = n;
    if (n > cap) return fail(RM_ERR_CAPACITY, "carry_out has room for fewer entries than the carry-out holds");
    return RM_OK;
}

int rm_csma_carry_collect_device(rm_context *c, int32_t n_ticks, const int32_t *const *dev_src, const int32_t *n_src, const int64_t *cca_time_us,
                                 const rm_csma_carry *carry, int32_t n_carry, const rm_csma_result *dev_out, const rm_csma_result *dev_carried_out,
                                 rm_csma_carry *carry_out, int64_t cap, int64_t *count)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    size_t n_pkt = 0;
    RM_TRY(collect_check(n_ticks, dev_src, n_src, cca_time_us, carry, n_carry, dev_out, dev_carried_out, carry_out, cap, &n_pkt));
    const size_t n_all = n_pkt + size_t(n_carry);
    if (count) *count = 0;
    if (n_all == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    rm_context::Energy::Csma &q = c->ed.cs;
    // what the kernels read, through the pinned block: the lists' places, the packets before each tick, the sample times, the carry-in
    const size_t off_first = pad64(size_t(n_ticks) * 8), off_cca = off_first + pad64((size_t(n_ticks) + 1) * 4);
    const size_t off_carry = off_cca + pad64(size_t(n_ticks) * 8), in_bytes = off_carry + pad64(size_t(n_carry) * sizeof(rm_csma_carry));
    const size_t n_out = std::min<size_t>(n_all, size_t(cap)), out_bytes = pad64(n_out * sizeof(rm_csma_carry));
    if (!q.h_collect || q.h_collect_in < in_bytes || q.h_collect_out < out_bytes) {
        if (q.h_collect) {
            RM_HIP(hipStreamSynchronize(c->stream));
            RM_HIP(hipHostFree(q.h_collect));
            q.h_collect = nullptr;
        }
        const size_t want_in = pad64(in_bytes + in_bytes / 2), want_out = pad64(out_bytes + out_bytes / 2);
        RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&q.h_collect), want_in + 64 + want_out, hipHostMallocMapped));
        q.h_collect_in = want_in;
        q.h_collect_out = want_out;
    }
    char *const h_in = q.h_collect;
    unsigned long long *const h_count = reinterpret_cast<unsigned long long *>(q.h_collect + q.h_collect_in);
    rm_csma_carry *const h_out = reinterpret_cast<rm_csma_carry *>(q.h_collect + q.h_collect_in + 64);
    int32_t *const h_first = reinterpret_cast<int32_t *>(h_in + off_first);
    std::memcpy(h_in, dev_src, size_t(n_ticks) * 8);
    h_first[0] = 0;
    for (int b = 0; b < n_ticks; ++b) h_first[b + 1] = h_first[b] + n_src[b];
    std::memcpy(h_in + off_cca, cca_time_us, size_t(n_ticks) * 8);
    if (n_carry > 0) std::memcpy(h_in + off_carry, carry, size_t(n_carry) * sizeof(rm_csma_carry));
    *h_count = 0ull;
    const size_t n_blocks = (n_all + 255) / 256;
    RM_HIP(q.collect_in.ensure(in_bytes));
    RM_HIP(q.collect_cnt.ensure(n_blocks));
    RM_HIP(hipMemcpyAsync(q.collect_in.p, h_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    rm::CsmaCollectDev cc{};
    cc.src = reinterpret_cast<const int32_t *const *>(q.collect_in.p);
    cc.own_first = reinterpret_cast<const int32_t *>(q.collect_in.p + off_first);
    cc.cca_us = reinterpret_cast<const int64_t *>(q.collect_in.p + off_cca);
    cc.carry = reinterpret_cast<const rm_csma_carry *>(q.collect_in.p + off_carry);
    cc.n_ticks = n_ticks;
    cc.n_pkt = int(n_pkt);
    cc.n_carry = n_carry;
    if (n_carry > 0) cc.status[0] = dev_carried_out->status, cc.attempts[0] = dev_carried_out->attempts, cc.tick[0] = dev_carried_out->tick;
    if (n_pkt > 0) cc.status[1] = dev_out->status, cc.attempts[1] = dev_out->attempts, cc.tick[1] = dev_out->tick;
    cc.block_cnt = q.collect_cnt.p;
    cc.h_out = h_out;
    cc.h_count = h_count;
    cc.cap = (long long)n_out;
    {
        CallProbe probe(c);
        sample_stage(probe.smp, RM_STAGE_SINR);
        RM_HIP(rm::launch_csma_collect(c->stream, cc));
    }
    RM_HIP(hipStreamSynchronize(c->stream)); // the one wait: the count and the records are in the pinned block
    const int64_t n = int64_t(*h_count);
    if (count) *count = n;
    if (n > cap) return fail(RM_ERR_CAPACITY, "carry_out has room for fewer entries than the carry-out holds");
    if (n > 0) std::memcpy(carry_out, h_out, size_t(n) * sizeof(rm_csma_carry));
    return RM_OK;
}

} // extern "C"
