// rm_api_listen.cpp -- C ABI: receiver listening schedules, duty-cycled radios on the device (the pass is
// rm_listen.hip).
//
// The tables belong to the context, not to a medium or a tick slot: one rm_listen_schedule and one missed count per node index.
// The evaluating calls run the pass (through the seam of rm_api_passes.cpp); everything here sets, clears and reads.
#include "rm_host.hpp"

using namespace rmh;

namespace rmh {

rm::ListenDev listen_dev(const rm_context *c)
{
    rm::ListenDev d{};
    d.sched = c->ls.sched.p;
    d.missed = c->ls.missed.p;
    d.n_nodes = c->ls.n;
    return d;
}

// off: every node always listens, the tables forgotten (the buffers stay for the next rm_listen_set)
static int listen_off(rm_context *c)
{
    rm_context::Listen &ls = c->ls;
    if (ls.n >= 0) RM_HIP(hipStreamSynchronize(c->stream)); // (a pass in flight still reads the tables; pointers handed out end here)
    ls.on = false;
    ls.n = -1;
    ls.host.clear();
    return RM_OK;
}

int listen_nodes_changed(rm_context *c)
{
    if (c->ls.n < 0 || c->ls.n == c->n) return RM_OK; // never set, or the same node count: both tables stay
    return listen_off(c);
}

// the tables for c->n nodes: every period 0, missed 0
static int listen_make(rm_context *c)
{
    rm_context::Listen &ls = c->ls;
    if (ls.n == c->n && ls.sched.p && ls.missed.p) return RM_OK;
    RM_HIP(hipStreamSynchronize(c->stream));
    RM_HIP(ls.sched.ensure(size_t(std::max(c->n, 1))));
    RM_HIP(ls.missed.ensure(size_t(std::max(c->n, 1))));
    RM_HIP(hipMemsetAsync(ls.sched.p, 0, size_t(std::max(c->n, 1)) * sizeof(rm_listen_schedule), c->stream));
    RM_HIP(hipMemsetAsync(ls.missed.p, 0, size_t(std::max(c->n, 1)) * sizeof(uint64_t), c->stream));
    ls.host.assign(size_t(c->n), rm_listen_schedule{0, 0, 0});
    ls.n = c->n;
    return RM_OK;
}

static int listen_have(const rm_context *c)
{
    if (c->ls.n < 0) return fail(RM_ERR_STATE, "no listening schedules: rm_listen_set comes first");
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_listen_set(rm_context *c, const int32_t *nodes, int32_t n, const rm_listen_schedule *sched)
{
    if (!c || n < 0 || (n > 0 && !sched)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(graphs_refuse(c, "the schedules' pass is not part of them"));
    // the whole list is validated before anything changes
    RM_TRY(check_node_list(nodes, n, c->n));
    for (int32_t k = 0; k < n; ++k)
        if (!rm::host_listen_valid(sched[k]))
            return fail(RM_ERR_INVALID, "bad rm_listen_schedule: period_us 0 with on_us = phase_us = 0, or period_us > 0 with "
                                        "0 <= on_us <= period_us and 0 <= phase_us < period_us");
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(ev_flush_append(c)); // (the tick before was evaluated under the old schedules: its append does not wait for the next drain)
    ev_touch(c);
    RM_TRY(listen_make(c));
    rm_context::Listen &ls = c->ls;
    if (!nodes) {
        if (n > 0) {
            std::memcpy(ls.host.data(), sched, size_t(n) * sizeof(rm_listen_schedule));
            // (from the host's copy, and waited for: neither the caller's array nor a later update of the copy can race with it)
            RM_HIP(hipMemcpyAsync(ls.sched.p, ls.host.data(), size_t(n) * sizeof(rm_listen_schedule), hipMemcpyHostToDevice, c->stream));
            RM_HIP(hipStreamSynchronize(c->stream));
        }
    } else if (n > 0) {
        // a list: applied to the host's copy in order (the last entry of a node wins), and every entry staged from that copy
        for (int32_t k = 0; k < n; ++k) ls.host[size_t(nodes[k])] = sched[k];
        RM_TRY(rows_write<rm_listen_schedule>(c, ls.h, ls.sched.p, ls.n, nodes, n, ls.host.data(), nodes));
    }
    ls.on = true;
    return RM_OK;
}

int rm_listen_get(rm_context *c, const int32_t *nodes, int32_t n, rm_listen_schedule *out)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(listen_have(c));
    RM_TRY(check_node_list(nodes, n, c->ls.n));
    for (int32_t k = 0; k < n; ++k) out[k] = c->ls.host[size_t(nodes ? nodes[k] : k)];
    return RM_OK;
}

int rm_listen_clear(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_HIP(hipSetDevice(c->device));
    if (c->ls.n >= 0) {
        RM_TRY(ev_flush_append(c));
        ev_touch(c);
    }
    return listen_off(c);
}

int rm_listen_enabled(const rm_context *c) { return (c && c->ls.on) ? 1 : 0; }

int rm_listen_missed_read(rm_context *c, const int32_t *nodes, int32_t n, uint64_t *out)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(listen_have(c));
    RM_TRY(check_node_list(nodes, n, c->ls.n));
    RM_HIP(hipSetDevice(c->device));
    return rows_read(c, c->ls.h, c->ls.missed.p, 1, c->ls.n, nodes, n, out, nullptr, nullptr);
}

int rm_listen_missed_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(listen_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(hipMemsetAsync(c->ls.missed.p, 0, size_t(std::max(c->ls.n, 1)) * sizeof(uint64_t), c->stream));
    return RM_OK;
}

int rm_listen_device(rm_context *c, const rm_listen_schedule **dev_sched, const uint64_t **dev_missed)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(listen_have(c));
    if (dev_sched) *dev_sched = c->ls.sched.p;
    if (dev_missed) *dev_missed = c->ls.missed.p;
    return RM_OK;
}

int rm_listen_at(const rm_listen_schedule *s, int64_t t_us)
{
    if (!s || !rm::host_listen_valid(*s)) return RM_ERR_INVALID;
    return rm::host_listen_at(*s, t_us) ? 1 : 0;
}

} // extern "C"
