// rm_api_linkest.cpp -- C ABI: link estimator, EWMA ETX over counter windows and forwarding acks on the device (DESIGN.md section
// 6, E23; the kernel is rm_linkest.hip).
//
// A fold READS a watch table and optionally a forwarding table -- the context's own (rm_api_linkstats.cpp, rm_api_fwd.cpp) or the
// caller's -- and writes only this feature's tables: the entries, the node state, the totals and the published table, which is a
// valid rm_etx_tables for the measured-route query.  No evaluating call reads or writes any of it.  Every check comes before the
// launch.  The host rule at the end is built from the same lest_* text of rm_math.hpp as the kernel.
#include "rm_host.hpp"
#include "rm_math.hpp"

using namespace rmh;

namespace rmh {

static const char *const kLestOff = "the link estimator is off: rm_linkest_enable comes first";

// what the feature keeps beside rm_context::Relay
static void linkest_free(rm_context *c)
{
    rm_context::LinkEst &le = c->le;
    le.K = 0;
    le.entry.release(); le.node.release(); le.pub_peer.release(); le.pub_stats.release(); le.totals.release();
    le.in_peer.release(); le.in_stats.release(); le.in_fwd.release();
}

int linkest_nodes_changed(rm_context *c) { return relay_nodes_changed(c, c->le, linkest_free); }
void linkest_release(rm_context *c) { relay_release(c, c->le, linkest_free); }

static bool lest_k_ok(int32_t K) { return K == 1 || K == 2 || K == 4 || K == 8; }

// the feature's own tables; the inputs are the fold's to fill in
static rm::LinkEstDev linkest_dev(const rm_context *c)
{
    const rm_context::LinkEst &le = c->le;
    rm::LinkEstDev f{};
    f.entry = le.entry.p;
    f.node = le.node.p;
    f.pub_peer = le.pub_peer.p;
    f.pub_stats = le.pub_stats.p;
    f.totals = le.totals.p;
    f.n_nodes = le.n;
    f.K = le.K;
    f.p = le.p;
    return f;
}

// explicit inputs: the struct's own rules (aligned: what the kernel's loads need of device pointers); K < 0: any valid K
static int lest_inputs_check(const rm_linkest_inputs *in, int32_t K, bool aligned)
{
    if (!lest_k_ok(in->K)) return fail(RM_ERR_INVALID, "inputs: K is 1, 2, 4 or 8");
    if (K >= 0 && in->K != K) return fail(RM_ERR_INVALID, "inputs: K is not the enabled K");
    if (in->reserved != 0) return fail(RM_ERR_INVALID, "inputs: reserved is not 0");
    if (!in->peer || !in->stats) return fail(RM_ERR_INVALID, "inputs: peer or stats is NULL");
    if (aligned && (reinterpret_cast<uintptr_t>(in->peer) % (4u * unsigned(in->K)) != 0 || reinterpret_cast<uintptr_t>(in->stats) % 8u != 0 ||
                    reinterpret_cast<uintptr_t>(in->fwd) % 8u != 0))
        return fail(RM_ERR_INVALID, "inputs: peer is not aligned to 4 K bytes, or stats or fwd not to 8");
    return RM_OK;
}

// what both fold forms refuse, arguments before state, before anything is launched or uploaded
static int linkest_fold_check(rm_context *c, const rm_linkest_inputs *in, bool aligned)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (in) RM_TRY(lest_inputs_check(in, c->le.on ? c->le.K : -1, aligned));
    RM_TRY(relay_have(c->le, kLestOff));
    if (c->in_tick) return fail(RM_ERR_STATE, "rm_linkest_fold between rm_tick_begin and rm_tick_flush");
    if (part_count(c) != c->n || part_spatial(c)) return fail(RM_ERR_STATE, "the link estimator does not run on a context with a receiver partition");
    if (c->le.n != c->n) return fail(RM_ERR_STATE, "internal: the link estimator's tables were made for another node count");
    if (!in) {
        if (!linkstats_on(c)) return fail(RM_ERR_STATE, "inputs is NULL and the watched-link statistics are off");
        if (c->lk.K != c->le.K) return fail(RM_ERR_STATE, "inputs is NULL and the watched-link statistics have another K: rm_linkest_enable with it");
        if (c->lk.n != c->le.n) return fail(RM_ERR_STATE, "internal: the watch table does not hold every node");
    }
    return RM_OK;
}

// the one launch, over checked inputs in device memory (in == nullptr: the context's own tables)
static int linkest_launch(rm_context *c, const rm_linkest_inputs *in)
{
    rm::LinkEstDev f = linkest_dev(c);
    if (in) {
        f.in_peer = in->peer;
        f.in_stats = in->stats;
        f.in_fwd = in->fwd;
    } else {
        f.in_peer = c->lk.peer.p;
        f.in_stats = c->lk.table.p;
        f.in_fwd = (c->fw.on && c->fw.n == c->le.n) ? c->fw.node.p : nullptr;
    }
    CallProbe probe(c); // (rm_profile_kernels names what ran)
    RM_HIP(rm::launch_linkest_fold(c->stream, f));
    return RM_OK;
}

} // namespace rmh

extern "C" {

void rm_linkest_defaults(rm_linkest_params *p)
{
    if (!p) return;
    *p = rm_linkest_params{3u, 5u, 230u, 230u, 6400u, 0u};
}

int rm_linkest_validate(const rm_linkest_params *p)
{
    if (!p) return fail(RM_ERR_INVALID, "params is NULL");
    if (!rm::lest_valid(*p))
        return fail(RM_ERR_INVALID, "bad rm_linkest_params: beacon_window and data_window 0 .. 2^31, both alphas 0 .. 255, max_etx 128 .. 65535, "
                                    "reserved 0");
    return RM_OK;
}

int rm_linkest_enable(rm_context *c, int32_t K, const rm_linkest_params *p)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(rm_linkest_validate(p));
    if (!lest_k_ok(K)) return fail(RM_ERR_INVALID, "K is 1, 2, 4 or 8");
    RM_TRY(graphs_refuse(c, "the extensions' tables are not set on it"));
    if (c->n < 1) return fail(RM_ERR_STATE, "no nodes: rm_nodes_upload comes first");
    if (part_count(c) != c->n || part_spatial(c)) return fail(RM_ERR_STATE, "the link estimator does not run on a context with a receiver partition");
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_off(c, c->le, linkest_free)); // (another enable: everything anew)
    rm_context::LinkEst &le = c->le;
    const size_t n = size_t(c->n), nk = n * size_t(K);
    hipError_t e = le.entry.ensure(nk);
    if (e == hipSuccess) e = le.node.ensure(n);
    if (e == hipSuccess) e = le.pub_peer.ensure(nk);
    if (e == hipSuccess) e = le.pub_stats.ensure(nk);
    if (e == hipSuccess) e = le.totals.ensure(1);
    if (e == hipSuccess) {
        le.p = *p;
        le.K = K;
        le.n = c->n;
        e = rm::launch_linkest_init(c->stream, linkest_dev(c));
    }
    if (e != hipSuccess) {
        linkest_release(c);
        return fail(RM_ERR_HIP, std::string("rm_linkest_enable: ") + hipGetErrorString(e));
    }
    le.on = true;
    return RM_OK;
}

int rm_linkest_disable(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_HIP(hipSetDevice(c->device));
    return relay_off(c, c->le, linkest_free);
}

int rm_linkest_enabled(const rm_context *c) { return (c && c->le.on) ? c->le.K : 0; }

int rm_linkest_get_params(const rm_context *c, rm_linkest_params *out)
{
    if (!c || !out) return fail(RM_ERR_INVALID, "ctx or out is NULL");
    RM_TRY(relay_have(c->le, kLestOff));
    *out = c->le.p;
    return RM_OK;
}

int rm_linkest_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(relay_have(c->le, kLestOff));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(rm::launch_linkest_init(c->stream, linkest_dev(c)));
    return RM_OK;
}

int rm_linkest_fold_device(rm_context *c, const rm_linkest_inputs *dev_inputs)
{
    RM_TRY(linkest_fold_check(c, dev_inputs, true));
    RM_HIP(hipSetDevice(c->device));
    return linkest_launch(c, dev_inputs);
}

int rm_linkest_fold(rm_context *c, const rm_linkest_inputs *inputs)
{
    RM_TRY(linkest_fold_check(c, inputs, false));
    RM_HIP(hipSetDevice(c->device));
    if (!inputs) return linkest_launch(c, nullptr);
    // the caller's arrays into the feature's device copies, which an earlier fold on the stream may still read
    rm_context::LinkEst &le = c->le;
    const size_t n = size_t(le.n), nk = n * size_t(le.K);
    RM_TRY(relay_room(c, le.in_peer, nk));
    RM_TRY(relay_room(c, le.in_stats, nk));
    if (inputs->fwd) RM_TRY(relay_room(c, le.in_fwd, n));
    RM_HIP(hipMemcpyAsync(le.in_peer.p, inputs->peer, nk * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipMemcpyAsync(le.in_stats.p, inputs->stats, nk * sizeof(rm_link_stats), hipMemcpyHostToDevice, c->stream));
    if (inputs->fwd) RM_HIP(hipMemcpyAsync(le.in_fwd.p, inputs->fwd, n * sizeof(rm_fwd_node), hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipStreamSynchronize(c->stream)); // (the caller's arrays are the caller's again)
    const rm_linkest_inputs dv{le.in_peer.p, le.in_stats.p, inputs->fwd ? le.in_fwd.p : nullptr, le.K, 0};
    return linkest_launch(c, &dv);
}

int rm_linkest_read(rm_context *c, const int32_t *nodes, int32_t n, rm_linkest_entry *entry_out, rm_linkest_node *node_out, rm_linkest_totals *totals)
{
    if (!c || n < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(relay_have(c->le, kLestOff));
    if (nodes || n != 0) RM_TRY(check_node_list(nodes, n, c->le.n));
    rm_context::LinkEst &le = c->le;
    RM_HIP(hipSetDevice(c->device));
    if (totals) RM_HIP(hipMemcpyAsync(totals, le.totals.p, sizeof(rm_linkest_totals), hipMemcpyDeviceToHost, c->stream));
    const int entry_words = int(sizeof(rm_linkest_entry) / 8) * le.K;
    if (entry_out && n > 0) RM_TRY(rows_read(c, le.h, le.entry.p, entry_words, le.n, nodes, n, entry_out, nullptr, nullptr));
    if (node_out && n > 0) RM_TRY(rows_read(c, le.h, le.node.p, int(sizeof(rm_linkest_node) / 8), le.n, nodes, n, node_out, nullptr, nullptr));
    RM_HIP(hipStreamSynchronize(c->stream));
    return RM_OK;
}

int rm_linkest_device(rm_context *c, const rm_linkest_entry **dev_entry, const rm_linkest_node **dev_node, const rm_linkest_totals **dev_totals)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(relay_have(c->le, kLestOff));
    if (dev_entry) *dev_entry = c->le.entry.p;
    if (dev_node) *dev_node = c->le.node.p;
    if (dev_totals) *dev_totals = c->le.totals.p;
    return RM_OK;
}

int rm_linkest_tables(rm_context *c, rm_etx_tables *out)
{
    if (!c || !out) return fail(RM_ERR_INVALID, "ctx or out is NULL");
    RM_TRY(relay_have(c->le, kLestOff));
    *out = rm_etx_tables{c->le.pub_peer.p, c->le.pub_stats.p, c->le.K, 0};
    return RM_OK;
}

int rm_linkest_fold_tables(int32_t n_nodes, const rm_linkest_inputs *inputs, const rm_linkest_params *params, rm_linkest_entry *entry,
                           rm_linkest_node *node, int32_t *pub_peer, rm_link_stats *pub_stats, rm_linkest_totals *totals)
{
    RM_TRY(rm_linkest_validate(params));
    if (!inputs) return fail(RM_ERR_INVALID, "inputs is NULL");
    if (n_nodes < 0) return fail(RM_ERR_INVALID, "n_nodes is negative");
    RM_TRY(lest_inputs_check(inputs, -1, false));
    if (n_nodes > 0 && (!entry || !node || !pub_peer || !pub_stats)) return fail(RM_ERR_INVALID, "a table is NULL");
    const rm_linkest_params &p = *params;
    const int32_t K = inputs->K;
    rm_linkest_totals t{};
    t.folds = 1;
    const bool data_on = inputs->fwd != nullptr && p.data_window > 0u;
    for (int32_t j = 0; j < n_nodes; ++j) {
        const size_t row = size_t(j) * size_t(K);
        uint32_t etx0[8];
        int32_t peer0[8];
        for (int32_t k = 0; k < K; ++k) {
            rm_linkest_entry &e = entry[row + size_t(k)];
            etx0[k] = e.etx;
            peer0[k] = e.peer;
            const rm_link_stats &st = inputs->stats[row + size_t(k)];
            const unsigned did = rm::lest_beacon(p, n_nodes, j, inputs->peer[row + size_t(k)], st.heard, st.delivered, e);
            if (did & rm::LEST_CLEARED) t.cleared += 1;
            if (did & rm::LEST_RESTARTED) {
                t.restarted += 1;
                node[j].restarted += 1u;
            }
            if (did & rm::LEST_SAMPLED) t.beacon_samples += 1;
        }
        if (data_on) {
            const rm_fwd_node &fw = inputs->fwd[j];
            uint64_t dT = 0, dA = 0;
            if (rm::lest_data(p, n_nodes, j, fw.next, fw.acked + fw.failed, fw.acked, node[j], dT, dA)) {
                int32_t k = 0;
                while (k < K && entry[row + size_t(k)].peer != fw.next) ++k;
                if (k == K) {
                    node[j].data_unmatched += 1u;
                    t.data_unmatched += 1;
                } else {
                    rm::lest_data_sample(p, dT, dA, entry[row + size_t(k)]);
                    node[j].data_samples += 1u;
                    t.data_samples += 1;
                }
            }
        }
        for (int32_t k = 0; k < K; ++k) {
            const rm_linkest_entry &e = entry[row + size_t(k)];
            t.estimates += uint64_t(int64_t(e.etx != 0u) - int64_t(etx0[k] != 0u));
            if (e.etx == etx0[k] && e.peer == peer0[k]) continue;
            pub_peer[row + size_t(k)] = e.peer;
            rm::lest_publish(e.etx, pub_stats[row + size_t(k)]);
        }
    }
    if (totals) {
        totals->folds += t.folds;
        totals->beacon_samples += t.beacon_samples;
        totals->data_samples += t.data_samples;
        totals->data_unmatched += t.data_unmatched;
        totals->restarted += t.restarted;
        totals->cleared += t.cleared;
        totals->estimates += t.estimates;
    }
    return RM_OK;
}

} // extern "C"
