// rm_api_flood.cpp -- C ABI: dissemination floods, Trickle-timed broadcast relay on the device (the
// kernels are rm_flood.hip).
//
// The table belongs to the context.  No evaluating call reads or writes it: the advance reads a FINISHED result slot through the
// unicast query's descriptor (uc_describe) and under its state rules (uc_check_state).  Every check comes before the first launch.
// What a relay feature's calls have in common -- rm_context::Relay and the relay_* helpers over it -- is at the end of rm_host.hpp.
#include "rm_host.hpp"
#include "rm_math.hpp"

using namespace rmh;

namespace rmh {

static const char *const kFloodOff = "dissemination floods are off: rm_flood_enable comes first";

// what the feature keeps beside rm_context::Relay
static void flood_free(rm_context *c)
{
    rm_context::Flood &fl = c->fl;
    fl.node.release(); fl.totals.release(); fl.pmin.release(); fl.tmin.release(); fl.act.release();
}

int flood_nodes_changed(rm_context *c) { return relay_nodes_changed(c, c->fl, flood_free); }
void flood_release(rm_context *c) { relay_release(c, c->fl, flood_free); }
static int flood_have(const rm_context *c) { return relay_have(c->fl, kFloodOff); }

static rm::FloodDev flood_dev(const rm_context *c)
{
    const rm_context::Flood &fl = c->fl;
    rm::FloodDev f{};
    f.node = fl.node.p;
    f.totals = fl.totals.p;
    f.claim = fl.claim.p;
    f.pmin = fl.pmin.p;
    f.tmin = fl.tmin.p;
    f.act = fl.act.p;
    f.n_nodes = fl.n;
    f.doublings = fl.p.doublings;
    f.max_intervals = fl.p.max_intervals;
    f.redundancy = fl.p.redundancy;
    f.max_hops = fl.p.max_hops;
    f.imin_us = fl.p.imin_us;
    f.seed = fl.p.seed;
    return f;
}

// the source list's three launches, for relay_sources_device / relay_sources
static auto flood_src_launch(rm_context *c, int64_t time_us, int32_t cap)
{
    return [=](int units, int chunk, int32_t *dev_src, int32_t *dev_count) {
        return rm::launch_flood_sources(c->stream, flood_dev(c), time_us, cap, units, chunk, c->fl.unit_count.p, dev_src, dev_count);
    };
}

} // namespace rmh

extern "C" {

void rm_flood_defaults(rm_flood_params *p)
{
    if (!p) return;
    *p = rm_flood_params{};
    p->imin_us = 8000;
    p->doublings = 4;
    p->max_intervals = 8;
    p->redundancy = 2;
    p->max_hops = 255;
    p->seed = 0;
}

int rm_flood_validate(const rm_flood_params *p)
{
    if (!p) return fail(RM_ERR_INVALID, "params is NULL");
    if (!rm::flood_valid(*p))
        return fail(RM_ERR_INVALID, "bad rm_flood_params: imin_us 2 .. 2^32, doublings 0 .. 16, max_intervals 1 .. 64, redundancy 0 .. 255, "
                                    "max_hops 1 .. 65535");
    return RM_OK;
}

int rm_flood_fire(const rm_flood_params *p, int32_t node, int64_t first_us, int32_t m, int64_t *start_us, int64_t *fire_us)
{
    if (!start_us || !fire_us) return fail(RM_ERR_INVALID, "start_us or fire_us is NULL");
    RM_TRY(rm_flood_validate(p));
    if (node < 0 || first_us < 0 || m < 0 || m > p->max_intervals) return fail(RM_ERR_INVALID, "node >= 0, first_us >= 0 and 0 <= m <= max_intervals");
    rm::flood_fire(p->imin_us, p->doublings, p->max_intervals, p->seed, node, first_us, m, *start_us, *fire_us);
    return RM_OK;
}

int rm_flood_enable(rm_context *c, const rm_flood_params *p)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(rm_flood_validate(p));
    RM_TRY(graphs_refuse(c, "the extensions' tables are not set on it"));
    if (c->n < 1) return fail(RM_ERR_STATE, "no nodes: rm_nodes_upload comes first");
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_off(c, c->fl, flood_free)); // (another enable: everything anew)
    rm_context::Flood &fl = c->fl;
    const size_t n = size_t(c->n);
    int units = 0, chunk = 0;
    rm::traffic_geometry(c->n, &units, &chunk);
    hipError_t e = fl.node.ensure(n);
    if (e == hipSuccess) e = fl.totals.ensure(1);
    if (e == hipSuccess) e = fl.claim.ensure(n);
    if (e == hipSuccess) e = fl.pmin.ensure(n);
    if (e == hipSuccess) e = fl.tmin.ensure(n);
    if (e == hipSuccess) e = fl.act.ensure(std::max<size_t>(n, 256)); // (a source list: at most n_nodes entries)
    if (e == hipSuccess) e = fl.unit_count.ensure(size_t(units));
    if (e == hipSuccess) {
        fl.p = *p;
        fl.n = c->n;
        e = rm::launch_flood_init(c->stream, flood_dev(c));
    }
    if (e != hipSuccess) {
        flood_release(c);
        return fail(RM_ERR_HIP, std::string("rm_flood_enable: ") + hipGetErrorString(e));
    }
    fl.on = true;
    return RM_OK;
}

int rm_flood_disable(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_HIP(hipSetDevice(c->device));
    return relay_off(c, c->fl, flood_free);
}

int rm_flood_enabled(const rm_context *c) { return (c && c->fl.on) ? 1 : 0; }

int rm_flood_get_params(const rm_context *c, rm_flood_params *out)
{
    if (!c || !out) return fail(RM_ERR_INVALID, "ctx or out is NULL");
    RM_TRY(flood_have(c));
    *out = c->fl.p;
    return RM_OK;
}

int rm_flood_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(flood_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(rm::launch_flood_init(c->stream, flood_dev(c)));
    return RM_OK;
}

int rm_flood_seed_device(rm_context *c, const int32_t *dev_nodes, int32_t n, int64_t time_us)
{
    if (!c || n < 0 || (n > 0 && !dev_nodes) || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(flood_have(c));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_room(c, c->fl.act, size_t(n)));
    CallProbe probe(c);
    RM_HIP(rm::launch_flood_seed(c->stream, flood_dev(c), dev_nodes, n, time_us));
    return RM_OK;
}

int rm_flood_seed(rm_context *c, const int32_t *nodes, int32_t n, int64_t time_us)
{
    if (!c || n < 0 || (n > 0 && !nodes) || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(flood_have(c));
    RM_TRY(relay_check_host_list(c->fl, nodes, n, "seed"));
    if (n == 0) return RM_OK;
    RM_TRY(relay_stage_list(c, c->fl, nodes, n));
    return rm_flood_seed_device(c, c->fl.stage.p, n, time_us);
}

int rm_flood_sources_device(rm_context *c, int64_t time_us, int32_t cap, int32_t *dev_src, int32_t *dev_count)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    return relay_sources_device(c, c->fl, kFloodOff, time_us, cap, dev_src, dev_count, flood_src_launch(c, time_us, cap));
}

int rm_flood_sources(rm_context *c, int64_t time_us, int32_t cap, int32_t *src, int32_t *count)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    return relay_sources(c, c->fl, kFloodOff, time_us, cap, src, count, flood_src_launch(c, time_us, cap));
}

int rm_flood_advance_device(rm_context *c, int32_t slot, const int32_t *dev_cand, int32_t n_cand)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    rm::UcSlot d;
    int32_t P = 0;
    RM_TRY(relay_advance_begin(c, c->fl, kFloodOff, slot, dev_cand, n_cand, &d, &P));
    RM_TRY(relay_room(c, c->fl.act, size_t(P)));
    CallProbe probe(c);
    RM_HIP(rm::launch_flood_advance(c->stream, flood_dev(c), d, dev_cand, P));
    return RM_OK;
}

int rm_flood_advance(rm_context *c, int32_t slot, const int32_t *cand, int32_t n_cand)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(relay_check_advance(c, c->fl, kFloodOff, slot, n_cand));
    if (cand) {
        RM_TRY(relay_check_host_list(c->fl, cand, n_cand, "candidate")); // (the forwarding queues' advance has no such check)
        RM_TRY(relay_stage_list(c, c->fl, cand, n_cand));
    }
    return rm_flood_advance_device(c, slot, cand ? c->fl.stage.p : nullptr, n_cand);
}

int rm_flood_read(rm_context *c, const int32_t *nodes, int32_t n, rm_flood_node *out, rm_flood_totals *totals)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(flood_have(c));
    if (nodes || n != 0) RM_TRY(check_node_list(nodes, n, c->fl.n));
    RM_HIP(hipSetDevice(c->device));
    if (totals) RM_HIP(hipMemcpyAsync(totals, c->fl.totals.p, sizeof(rm_flood_totals), hipMemcpyDeviceToHost, c->stream));
    RM_TRY(rows_read(c, c->fl.h, c->fl.node.p, sizeof(rm_flood_node) / 8, c->fl.n, nodes, n, out, nullptr, nullptr));
    return RM_OK;
}

int rm_flood_device(rm_context *c, const rm_flood_node **dev_node, const rm_flood_totals **dev_totals)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(flood_have(c));
    if (dev_node) *dev_node = c->fl.node.p;
    if (dev_totals) *dev_totals = c->fl.totals.p;
    return RM_OK;
}

int rm_flood_tree_device(rm_context *c, int32_t *dev_parent, int32_t *dev_hop)
{
    if (!c || !dev_parent) return fail(RM_ERR_INVALID, "ctx or dev_parent is NULL");
    RM_TRY(flood_have(c));
    RM_HIP(hipSetDevice(c->device));
    CallProbe probe(c);
    RM_HIP(rm::launch_flood_tree(c->stream, flood_dev(c), dev_parent, dev_hop));
    return RM_OK;
}

} // extern "C"
