// rm_api_fwd.cpp -- C ABI: forwarding queues, multi-hop packet relay on the device (the kernels are
// rm_fwd.hip).
//
// The tables belong to the context.  No evaluating call reads or writes them: the advance reads a FINISHED result slot through the
// unicast query's descriptor (uc_describe) and under its state rules (uc_check_state).  Every check comes before the first launch.
// What a relay feature's calls have in common -- rm_context::Relay and the relay_* helpers over it -- is at the end of rm_host.hpp.
#include "rm_host.hpp"
#include "rm_math.hpp"

using namespace rmh;

namespace rmh {

static const char *const kFwdOff = "forwarding queues are off: rm_fwd_enable comes first";

// what the feature keeps beside rm_context::Relay
static void fwd_free(rm_context *c)
{
    rm_context::Fwd &fw = c->fw;
    fw.node.release(); fw.pk.release(); fw.totals.release(); fw.acc.release(); fw.pushed.release(); fw.act.release();
}

int fwd_nodes_changed(rm_context *c) { return relay_nodes_changed(c, c->fw, fwd_free); }
void fwd_release(rm_context *c) { relay_release(c, c->fw, fwd_free); }
static int fwd_have(const rm_context *c) { return relay_have(c->fw, kFwdOff); }

static rm::FwdDev fwd_dev(const rm_context *c)
{
    const rm_context::Fwd &fw = c->fw;
    rm::FwdDev f{};
    f.node = fw.node.p;
    f.pk = fw.pk.p;
    f.totals = fw.totals.p;
    f.claim = fw.claim.p;
    f.acc = fw.acc.p;
    f.pushed = fw.pushed.p;
    f.act = fw.act.p;
    f.n_nodes = fw.n;
    f.Q = fw.p.queue_slots;
    f.max_retries = fw.p.max_retries;
    f.min_be = fw.p.min_be;
    f.max_be = fw.p.max_be;
    f.max_hops = fw.p.max_hops;
    f.unit_us = fw.p.backoff_unit_us;
    f.seed = fw.p.seed;
    return f;
}

// the source list's three launches, for relay_sources_device / relay_sources
static auto fwd_src_launch(rm_context *c, int64_t time_us, int32_t cap)
{
    return [=](int units, int chunk, int32_t *dev_src, int32_t *dev_count) {
        return rm::launch_fwd_sources(c->stream, fwd_dev(c), time_us, cap, units, chunk, c->fw.unit_count.p, dev_src, dev_count);
    };
}

} // namespace rmh

extern "C" {

void rm_fwd_defaults(rm_fwd_params *p)
{
    if (!p) return;
    *p = rm_fwd_params{};
    p->queue_slots = 8;
    p->max_retries = 3;
    p->min_be = 3;
    p->max_be = 5;
    p->max_hops = 64;
    p->backoff_unit_us = 320;
    p->seed = 0;
}

int rm_fwd_validate(const rm_fwd_params *p)
{
    if (!p) return fail(RM_ERR_INVALID, "params is NULL");
    if (!rm::fwd_valid(*p))
        return fail(RM_ERR_INVALID, "bad rm_fwd_params: queue_slots 1, 2, 4, 8 or 16, max_retries 0 .. 15, 0 <= min_be <= max_be <= 8, max_hops 1 .. 255, "
                                    "backoff_unit_us 0 .. 2^32, reserved 0");
    return RM_OK;
}

int rm_fwd_backoff(const rm_fwd_params *p, int32_t node, int64_t start_us, int32_t tries, int64_t *delay_us)
{
    if (!delay_us) return fail(RM_ERR_INVALID, "delay_us is NULL");
    RM_TRY(rm_fwd_validate(p));
    if (node < 0 || start_us < 0 || tries < 1) return fail(RM_ERR_INVALID, "node >= 0, start_us >= 0 and tries >= 1");
    *delay_us = int64_t(rm::fwd_backoff_factor(p->seed, p->min_be, p->max_be, node, start_us, tries)) * p->backoff_unit_us;
    return RM_OK;
}

int rm_fwd_enable(rm_context *c, const rm_fwd_params *p)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(rm_fwd_validate(p));
    RM_TRY(graphs_refuse(c, "the extensions' tables are not set on it"));
    if (c->n < 1) return fail(RM_ERR_STATE, "no nodes: rm_nodes_upload comes first");
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_off(c, c->fw, fwd_free)); // (another enable: everything anew)
    rm_context::Fwd &fw = c->fw;
    const size_t n = size_t(std::max(c->n, 1));
    hipError_t e = fw.node.ensure(n);
    if (e == hipSuccess) e = fw.pk.ensure(n * size_t(p->queue_slots));
    if (e == hipSuccess) e = fw.totals.ensure(1);
    if (e == hipSuccess) e = fw.claim.ensure(n);
    if (e == hipSuccess) e = fw.acc.ensure(n);
    if (e == hipSuccess) e = fw.pushed.ensure(n);
    int units = 0, chunk = 0;
    rm::traffic_geometry(c->n, &units, &chunk);
    if (e == hipSuccess) e = fw.act.ensure(std::max<size_t>(n, 256)); // (a source list, a traffic row: at most n_nodes entries)
    if (e == hipSuccess) e = fw.unit_count.ensure(size_t(units));
    if (e == hipSuccess) e = hipMemsetAsync(fw.pk.p, 0, n * size_t(p->queue_slots) * sizeof(rm_fwd_packet), c->stream);
    if (e == hipSuccess) {
        fw.p = *p;
        fw.n = c->n;
        e = rm::launch_fwd_init(c->stream, fwd_dev(c), false);
    }
    if (e != hipSuccess) {
        fwd_release(c);
        return fail(RM_ERR_HIP, std::string("rm_fwd_enable: ") + hipGetErrorString(e));
    }
    fw.on = true;
    return RM_OK;
}

int rm_fwd_disable(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_HIP(hipSetDevice(c->device));
    return relay_off(c, c->fw, fwd_free);
}

int rm_fwd_enabled(const rm_context *c) { return (c && c->fw.on) ? 1 : 0; }

int rm_fwd_get_params(const rm_context *c, rm_fwd_params *out)
{
    if (!c || !out) return fail(RM_ERR_INVALID, "ctx or out is NULL");
    RM_TRY(fwd_have(c));
    *out = c->fw.p;
    return RM_OK;
}

int rm_fwd_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(fwd_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(hipMemsetAsync(c->fw.pk.p, 0, size_t(std::max(c->fw.n, 1)) * size_t(c->fw.p.queue_slots) * sizeof(rm_fwd_packet), c->stream));
    RM_HIP(rm::launch_fwd_init(c->stream, fwd_dev(c), true));
    return RM_OK;
}

int rm_fwd_set_next_device(rm_context *c, const int32_t *dev_parent, const int32_t *dev_roots, int32_t n_roots, int64_t time_us)
{
    if (!c || !dev_parent || n_roots < 0 || (n_roots > 0 && !dev_roots) || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(fwd_have(c));
    RM_HIP(hipSetDevice(c->device));
    CallProbe probe(c);
    RM_HIP(rm::launch_fwd_set_next(c->stream, fwd_dev(c), dev_parent, dev_roots, n_roots, time_us));
    return RM_OK;
}

int rm_fwd_set_next(rm_context *c, const int32_t *parent, const int32_t *roots, int32_t n_roots, int64_t time_us)
{
    if (!c || !parent || n_roots < 0 || (n_roots > 0 && !roots) || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(fwd_have(c));
    RM_TRY(relay_check_host_list(c->fw, roots, n_roots, "roots"));
    RM_HIP(hipSetDevice(c->device));
    const size_t n = size_t(c->fw.n);
    RM_TRY(relay_room(c, c->fw.stage, n + size_t(n_roots)));
    int32_t *d = c->fw.stage.p;
    if (n > 0) RM_HIP(hipMemcpyAsync(d, parent, n * 4, hipMemcpyHostToDevice, c->stream));
    if (n_roots > 0) RM_HIP(hipMemcpyAsync(d + n, roots, size_t(n_roots) * 4, hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipStreamSynchronize(c->stream));
    return rm_fwd_set_next_device(c, d, n_roots > 0 ? d + n : nullptr, n_roots, time_us);
}

int rm_fwd_inject_device(rm_context *c, const int32_t *dev_src, int32_t n, int64_t time_us)
{
    if (!c || n < 0 || (n > 0 && !dev_src) || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(fwd_have(c));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_room(c, c->fw.act, size_t(n)));
    CallProbe probe(c);
    RM_HIP(rm::launch_fwd_inject(c->stream, fwd_dev(c), dev_src, n, time_us));
    return RM_OK;
}

int rm_fwd_inject(rm_context *c, const int32_t *src, int32_t n, int64_t time_us)
{
    if (!c || n < 0 || (n > 0 && !src) || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(fwd_have(c));
    RM_TRY(relay_check_host_list(c->fw, src, n, "source"));
    if (n == 0) return RM_OK;
    RM_TRY(relay_stage_list(c, c->fw, src, n));
    return rm_fwd_inject_device(c, c->fw.stage.p, n, time_us);
}

int rm_fwd_sources_device(rm_context *c, int64_t time_us, int32_t cap, int32_t *dev_src, int32_t *dev_count)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    return relay_sources_device(c, c->fw, kFwdOff, time_us, cap, dev_src, dev_count, fwd_src_launch(c, time_us, cap));
}

int rm_fwd_sources(rm_context *c, int64_t time_us, int32_t cap, int32_t *src, int32_t *count)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    return relay_sources(c, c->fw, kFwdOff, time_us, cap, src, count, fwd_src_launch(c, time_us, cap));
}

int rm_fwd_advance_device(rm_context *c, int32_t slot, const int32_t *dev_cand, int32_t n_cand)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    rm::UcSlot d;
    int32_t P = 0;
    RM_TRY(relay_advance_begin(c, c->fw, kFwdOff, slot, dev_cand, n_cand, &d, &P));
    RM_TRY(relay_room(c, c->fw.act, size_t(P)));
    CallProbe probe(c);
    RM_HIP(rm::launch_fwd_advance(c->stream, fwd_dev(c), d, dev_cand, P));
    return RM_OK;
}

int rm_fwd_advance(rm_context *c, int32_t slot, const int32_t *cand, int32_t n_cand)
{
    if (!c) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(relay_check_advance(c, c->fw, kFwdOff, slot, n_cand));
    // (no bound check of the host list, unlike the flood's: k_fwd_adv_claim treats a candidate outside the table as foreign)
    if (cand) RM_TRY(relay_stage_list(c, c->fw, cand, n_cand));
    return rm_fwd_advance_device(c, slot, cand ? c->fw.stage.p : nullptr, n_cand);
}

int rm_fwd_read(rm_context *c, const int32_t *nodes, int32_t n, rm_fwd_node *out, rm_fwd_totals *totals)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(fwd_have(c));
    if (nodes || n != 0) RM_TRY(check_node_list(nodes, n, c->fw.n));
    RM_HIP(hipSetDevice(c->device));
    if (totals) RM_HIP(hipMemcpyAsync(totals, c->fw.totals.p, sizeof(rm_fwd_totals), hipMemcpyDeviceToHost, c->stream));
    RM_TRY(rows_read(c, c->fw.h, c->fw.node.p, sizeof(rm_fwd_node) / 8, c->fw.n, nodes, n, out, nullptr, nullptr));
    for (int32_t k = 0; k < n; ++k) out[k].slot_mask = 0u; // (slot positions are not observable: they follow the atomics' order)
    return RM_OK;
}

int rm_fwd_queue_read(rm_context *c, const int32_t *nodes, int32_t n, rm_fwd_packet *out, int32_t *len)
{
    if (!c || n < 0 || (n > 0 && (!out || !len))) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(fwd_have(c));
    RM_TRY(check_node_list(nodes, n, c->fw.n));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    const int Q = c->fw.p.queue_slots;
    static thread_local std::vector<rm_fwd_node> rows;
    rows.resize(size_t(n));
    RM_TRY(rows_read(c, c->fw.h, c->fw.node.p, sizeof(rm_fwd_node) / 8, c->fw.n, nodes, n, rows.data(), nullptr, nullptr));
    RM_TRY(rows_read(c, c->fw.h, c->fw.pk.p, 3 * Q, c->fw.n, nodes, n, out, nullptr, nullptr));
    for (int32_t k = 0; k < n; ++k) { // the occupied slots to the front, in queue order; the rest zeroed
        rm_fwd_packet *q = out + size_t(k) * size_t(Q);
        int m = 0;
        for (int s = 0; s < Q; ++s)
            if ((rows[size_t(k)].slot_mask >> s) & 1u) q[m++] = q[s];
        std::sort(q, q + m, rm::fwd_packet_order);
        for (int s = m; s < Q; ++s) q[s] = rm_fwd_packet{};
        len[k] = m;
    }
    return RM_OK;
}

int rm_fwd_device(rm_context *c, const rm_fwd_node **dev_node, const rm_fwd_packet **dev_packets, const rm_fwd_totals **dev_totals)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(fwd_have(c));
    if (dev_node) *dev_node = c->fw.node.p;
    if (dev_packets) *dev_packets = c->fw.pk.p;
    if (dev_totals) *dev_totals = c->fw.totals.p;
    return RM_OK;
}

} // extern "C"
