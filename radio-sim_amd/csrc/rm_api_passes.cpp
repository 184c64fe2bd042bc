// rm_api_passes.cpp -- the passes over a finished result: the frame error model (E10), the listening schedules (E13), the traffic
// counters (E11) and the watched-link statistics (E14).  DESIGN.md section 6 states the order: each pass reads the verdicts the
// one before it left.  The table below holds it, and every route runs the passes through here: a lone or dense tick
// (launch_tick), a batch (launch_batch), a batch launched tick by tick (batch_run's fallback).
#include "rm_host.hpp"

using namespace rmh;

namespace {

struct Pass {
    bool (*on)(const rm_context *);
    bool sinr_only; // runs over the SINR medium's results only
    // the refusals' words: "<is_on>: ... do not run <its_pass> (<off_hint>)"; the internal error's: "<owner> pass cannot run ..."
    const char *is_on, *its_pass, *off_hint, *owner;
    hipError_t (*tick)(hipStream_t, const rm_context *, const rm::TickDev &);
    hipError_t (*batch)(hipStream_t, const rm_context *, int, const rm::TickDev *);
};

// in the order the passes run
const Pass kPasses[] = {
    {em_on, true, "the frame error model is on", "its pass", "rm_set_error_model with RM_EM_NONE switches it off", "the frame error model's",
     [](hipStream_t s, const rm_context *c, const rm::TickDev &t) { return rm::launch_errmodel(s, em_dev(c), t); },
     [](hipStream_t s, const rm_context *c, int n, const rm::TickDev *d) { return rm::launch_errmodel_batch(s, em_dev(c), n, d); }},
    {listen_on, false, "listening schedules are on", "their pass", "rm_listen_clear switches them off", "the listening schedules'",
     [](hipStream_t s, const rm_context *c, const rm::TickDev &t) { return rm::launch_listen(s, listen_dev(c), t); },
     [](hipStream_t s, const rm_context *c, int n, const rm::TickDev *d) { return rm::launch_listen_batch(s, listen_dev(c), n, d); }},
    {stats_on, false, "statistics are on", "the counters' pass", "rm_stats_enable with 0 switches them off", "the traffic counters'",
     [](hipStream_t s, const rm_context *c, const rm::TickDev &t) { return rm::launch_stats(s, stats_dev(c), t); },
     [](hipStream_t s, const rm_context *c, int n, const rm::TickDev *d) { return rm::launch_stats_batch(s, stats_dev(c), n, d); }},
    {linkstats_on, false, "watched-link statistics are on", "their pass", "rm_linkstats_enable with 0 switches them off",
     "the watched-link statistics'",
     [](hipStream_t s, const rm_context *c, const rm::TickDev &t) { return rm::launch_linkstats(s, linkstats_dev(c), t); },
     [](hipStream_t s, const rm_context *c, int n, const rm::TickDev *d) { return rm::launch_linkstats_batch(s, linkstats_dev(c), n, d); }},
};
// the refusals are asked in the order of the extensions' numbers (E10, E11, E13, E14): which of them a caller with several passes
// on is told about is part of what the calls promise
const int kRefusalOrder[] = {0, 2, 1, 3};

int refuse(const Pass &p, const rm_context *c, bool gathered)
{
    if (!p.on(c)) return RM_OK;
    if (gathered)
        return fail(RM_ERR_STATE, std::string(p.is_on) + ": the gathered, rm_dist_* and rm_group_* forms do not run " + p.its_pass + " (" +
                                      p.off_hint + ")");
    if (part_spatial(c) || part_count(c) != c->n)
        return fail(RM_ERR_STATE, std::string(p.is_on) + ": a context with a receiver partition does not run " + p.its_pass);
    return RM_OK;
}

} // namespace

namespace rmh {

int passes_check(const rm_context *const *members, size_t n, bool gathered, bool with_em)
{
    for (int k : kRefusalOrder) {
        if (kPasses[k].sinr_only && !with_em) continue;
        for (size_t r = 0; r < n; ++r) RM_TRY(refuse(kPasses[k], members[r], gathered));
    }
    return RM_OK;
}

int passes_check(const rm_context *c, bool gathered, bool with_em)
{
    return passes_check(&c, 1, gathered, with_em);
}

bool passes_counting(const rm_context *c)
{
    for (const Pass &p : kPasses)
        if (!p.sinr_only && p.on(c)) return true;
    return false;
}

int passes_tick(rm_context *c, TickSlot &ts, rm_context::Sample *smp, bool sinr)
{
    bool first = true;
    for (const Pass &p : kPasses) {
        if (!p.on(c) || (p.sinr_only && !sinr)) continue;
        if (first) {
            if (ts.draws_pending)
                return fail(RM_ERR_STATE, std::string("internal: ") + p.owner + " pass cannot run before the ranks' draws are finished");
            // the tick's compact arrays at once (a dense tick: its records from the lane masks), then the passes over them -- on the
            // stream before the hand-over to the reception stage (run_tick), before any pack launch and any copy, which all read
            // out_verdict from here on
            sample_stage(smp, RM_STAGE_REORDER);
            RM_TRY(materialize(c, ts));
            first = false;
        }
        sample_stage(smp, p.sinr_only ? RM_STAGE_SINR : RM_STAGE_REORDER);
        RM_HIP(p.tick(c->stream, c, ts.last));
    }
    // the masks of a dense tick carry one verdict per packet and cannot express the schedules' pass: rm_result_dense refuses the tick
    // (the counters leave the masks as they are: it keeps answering)
    if (ts.dense_result && listen_on(c)) ts.dense_listen = true;
    return RM_OK;
}

int passes_batch(rm_context *c, int n, const rm::TickDev *dev_ticks, rm_context::Sample *smp, int counters_stage)
{
    // every verdict of the batch is final here (the draws, the interference stages of a batch of overlapping ticks); ONE launch per
    // pass over all slots, ahead of everything that reads them (result copies, the packing launch of rm_batch_result_view,
    // rm_events_process_batch)
    for (const Pass &p : kPasses) {
        if (!p.on(c) || (p.sinr_only && !is_sinr(c))) continue;
        sample_stage(smp, p.sinr_only ? RM_STAGE_SINR : counters_stage);
        RM_HIP(p.batch(c->stream, c, n, dev_ticks));
    }
    return RM_OK;
}

int passes_nodes_changed(rm_context *c)
{
    RM_TRY(stats_nodes_changed(c));
    RM_TRY(listen_nodes_changed(c));
    RM_TRY(traffic_nodes_changed(c));
    RM_TRY(fwd_nodes_changed(c));
    RM_TRY(flood_nodes_changed(c));
    RM_TRY(linkest_nodes_changed(c));
    return linkstats_nodes_changed(c);
}

void passes_release(rm_context *c)
{
    c->st.table.release(); c->st.totals.release(); c->st.h.release();
    c->ls.sched.release(); c->ls.missed.release(); c->ls.h.release();
    traffic_release(c);
    linkstats_release(c);
    neighbors_release(c);
    hops_release(c);
    routes_release(c);
    etx_release(c);
    fwd_release(c);
    flood_release(c);
    nbtable_release(c);
    linkest_release(c);
}

} // namespace rmh
