// rm_api_csma.cpp -- C ABI: the CSMA-CA gated batch (rm_batch_run_sources_csma*, rm_csma_schedule; rm_csma.hip).
//
// A deferred candidate backs off and senses again in a later tick of the same batch.  The backoff draw is a hash of the packet and the
// attempt number, so the host lays out every attempt of every packet before anything is launched (csma_schedule): attempts are extra
// slots of their ticks' lists.  The gate then is the gated batch's (rm_api_cca.cpp) over those expanded lists, with one state per
// packet in the serial pass, and the unchanged batch runs over the gated expanded lists.
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

// counts only (fill = false: n_exp, first, own_first, total), or the slots too.  Packets are walked in (origin tick, origin slot) order,
// and a packet has at most one attempt per tick: appending to the ticks' cursors leaves every tick's retries in that order.
void csma_schedule(const rm_csma_params &p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us, Schedule &s, bool fill)
{
    const uint64_t seed_mixed = rm::host_mix64(p.seed + 0x9E3779B97F4A7C15ull);
    s.n_exp.assign(n_src, n_src + n_ticks);
    s.own_first.assign(size_t(n_ticks) + 1, 0);
    for (int b = 0; b < n_ticks; ++b) s.own_first[size_t(b) + 1] = s.own_first[size_t(b)] + n_src[b];
    for (int pass = 0; pass < (fill ? 2 : 1); ++pass) {
        std::vector<int32_t> cursor;
        if (pass == 1) {
            s.origin.resize(size_t(s.total));
            s.next_tick.resize(size_t(s.total));
            s.attempt.resize(size_t(s.total));
            cursor.resize(size_t(n_ticks));
            for (int b = 0; b < n_ticks; ++b) cursor[size_t(b)] = s.first[size_t(b)] + n_src[b];
        }
        for (int b = 0; b < n_ticks; ++b) {
            const uint64_t h1 = rm::host_mix64(seed_mixed ^ uint64_t(cca_time_us[b]));
            for (int32_t k = 0; k < n_src[b]; ++k) {
                int64_t tick = b;
                int32_t slot = pass == 1 ? s.first[size_t(b)] + k : 0;
                for (int a = 0; a <= p.max_backoffs; ++a) {
                    const int64_t next = a < p.max_backoffs ? csma_next_tick(p, h1, k, a, tick) : -1;
                    if (pass == 1) {
                        s.origin[size_t(slot)] = s.own_first[size_t(b)] + k;
                        s.attempt[size_t(slot)] = uint8_t(a);
                        s.next_tick[size_t(slot)] = int32_t(next);
                    }
                    if (next < 0 || next >= n_ticks) break;
                    tick = next;
                    if (pass == 0) ++s.n_exp[size_t(tick)];
                    else slot = cursor[size_t(tick)]++;
                }
            }
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

// a packet contributes at most 1 + max_backoffs <= 6 slots: with at most 2^27 packets the slot count stays below the 2^30 the
// pair list's slot field holds
constexpr size_t kCsmaMaxPackets = size_t(1) << 27;

// what both forms refuse, before anything is launched and with nothing changed; leaves the schedule in `s`
int csma_check(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src, const int32_t *n_src,
               const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us, const rm_csma_params *p, Schedule &s)
{
    RM_TRY(cca_batch_check_lists(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us));
    RM_TRY(csma_params_check(p));
    size_t n_pkt = 0;
    for (int b = 0; b < n_ticks; ++b) n_pkt += size_t(n_src[b]);
    if (n_pkt > kCsmaMaxPackets) return fail(RM_ERR_CAPACITY, "more than 2^27 packets in one CSMA-CA gated batch");
    csma_schedule(*p, n_ticks, n_src, cca_time_us, s, true);
    return cca_batch_check_ticks(c, n_ticks, t_begin_us, s.n_exp.data(), start_us, air_us, cca_time_us);
}

// src[b] and out's pointers: device-visible memory
int csma_batch(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src, const int32_t *n_src,
               const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us, double cca_threshold, const Schedule &s,
               const rm_csma_result *out, int32_t *n_exp)
{
    RM_HIP(hipSetDevice(c->device));
    const size_t n_slots = size_t(s.total), n_pkt = size_t(s.own_first[size_t(n_ticks)]);
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
        const size_t bytes = off_att + pad64(n_slots);
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
        RM_HIP(q.sched.ensure(bytes));
        RM_HIP(q.state.ensure(std::max<size_t>(n_pkt, 1)));
        RM_HIP(q.tentative.ensure(n_slots));
        RM_HIP(q.slot_flags.ensure(n_slots));
        RM_HIP(hipMemcpyAsync(q.sched.p, h_up, bytes, hipMemcpyHostToDevice, c->stream));
        cs.origin = reinterpret_cast<const int32_t *>(q.sched.p);
        cs.next_tick = reinterpret_cast<const int32_t *>(q.sched.p + off_next);
        cs.own_first = reinterpret_cast<const int32_t *>(q.sched.p + off_own);
        cs.attempt = reinterpret_cast<const uint8_t *>(q.sched.p + off_att);
        cs.n_pkt = int(n_pkt);
        cs.state = q.state.p;
        cs.tentative = q.tentative.p;
        cs.slot_flags = q.slot_flags.p;
        if (out) cs.out = *out;
        rm::ModelDev m = model_dev(c);
        if (c->f32_slack > 0.05) m.shadow_tbl = nullptr; // (as the query: the link-hash table goes with the fp32 filter of a small frame)
        {
            // profiling (rm_profile_kernels names the kernels that ran); the gate does not move the ticks' sampling on
            const uint64_t tick_index = c->tick_index;
            ProbeScope probe(c);
            c->tick_index = tick_index;
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
    if (n_exp) std::memcpy(n_exp, s.n_exp.data(), size_t(n_ticks) * 4);
    // the unchanged batch over the gated expanded lists (a batch without packets keeps its NULL lists)
    const int rc = batch_run(c, n_ticks, t_begin_us, t_end_us, gated_v.data(), nullptr, s.n_exp.data(), start_us, air_us);
    ev_batch_ran(c, rc, n_ticks, true);
    return rc;
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

int rm_csma_schedule(const rm_csma_params *p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us, int32_t *n_exp, int32_t *origin,
                     uint8_t *attempt, int64_t cap, int64_t *total)
{
    RM_TRY(csma_params_check(p));
    if (n_ticks < 1 || n_ticks > RM_MAX_BATCH || !n_src || !cca_time_us || cap < 0) return fail(RM_ERR_INVALID, "bad arguments");
    size_t n_pkt = 0;
    for (int b = 0; b < n_ticks; ++b) {
        if (n_src[b] < 0) return fail(RM_ERR_INVALID, "bad arguments");
        n_pkt += size_t(n_src[b]);
    }
    if (n_pkt > kCsmaMaxPackets) return fail(RM_ERR_CAPACITY, "more than 2^27 packets in one CSMA-CA gated batch");
    static thread_local Schedule s;
    const bool fill = origin != nullptr || attempt != nullptr;
    csma_schedule(*p, n_ticks, n_src, cca_time_us, s, false);
    if (n_exp) std::memcpy(n_exp, s.n_exp.data(), size_t(n_ticks) * 4);
    if (total) *total = s.total;
    if (!fill) return RM_OK;
    if (cap < s.total) return fail(RM_ERR_CAPACITY, "origin / attempt have room for fewer entries than the expanded lists hold");
    csma_schedule(*p, n_ticks, n_src, cca_time_us, s, true);
    if (origin && s.total > 0) std::memcpy(origin, s.origin.data(), size_t(s.total) * 4);
    if (attempt && s.total > 0) std::memcpy(attempt, s.attempt.data(), size_t(s.total));
    return RM_OK;
}

int rm_batch_run_sources_csma_device(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *dev_src,
                                     const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                                     double cca_threshold_dbm, const rm_csma_params *p, const rm_csma_result *dev_out, int32_t *n_exp)
{
    static thread_local Schedule s;
    RM_TRY(csma_check(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us, p, s));
    return csma_batch(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, s, dev_out, n_exp);
}

int rm_batch_run_sources_csma(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                              const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                              double cca_threshold_dbm, const rm_csma_params *p, const rm_csma_result *out, int32_t *n_exp)
{
    static thread_local Schedule s;
    RM_TRY(csma_check(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us, p, s));
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
    rm_csma_result dev{};
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
    RM_TRY(csma_batch(c, n_ticks, t_begin_us, t_end_us, lists.data(), n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, s, &dev, n_exp));
    RM_HIP(hipStreamSynchronize(c->stream));
    if (total > 0 && out) {
        if (out->status) RM_HIP(hipMemcpy(out->status, dev.status, total, hipMemcpyDeviceToHost));
        if (out->attempts) RM_HIP(hipMemcpy(out->attempts, dev.attempts, total, hipMemcpyDeviceToHost));
        if (out->tick) RM_HIP(hipMemcpy(out->tick, dev.tick, total * 4, hipMemcpyDeviceToHost));
        if (out->pkt) RM_HIP(hipMemcpy(out->pkt, dev.pkt, total * 4, hipMemcpyDeviceToHost));
        if (out->flags) RM_HIP(hipMemcpy(out->flags, dev.flags, total, hipMemcpyDeviceToHost));
        if (out->energy_dbm) RM_HIP(hipMemcpy(out->energy_dbm, dev.energy_dbm, total * 8, hipMemcpyDeviceToHost));
    }
    return RM_OK;
}

} // extern "C"
