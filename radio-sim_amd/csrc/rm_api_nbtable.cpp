// rm_api_nbtable.cpp -- C ABI: neighbour tables, discover / evict / expire watched peers on the device (DESIGN.md section 6, E22;
// the kernels are rm_nbtable.hip).
//
// The peers and entries are the watched-link statistics' tables (rm_api_linkstats.cpp); the counters and one word of scratch per
// node belong to this feature.  No evaluating call reads or writes any of it: the update reads a FINISHED result slot through the
// unicast query's descriptor (uc_describe) and under the relay features' state rules (relay_check_advance).  Every check comes
// before the first launch.  The host rule at the end is built from the same nbt_* text of rm_math.hpp as the kernels.
#include "rm_host.hpp"
#include "rm_math.hpp"

using namespace rmh;

namespace rmh {

static const char *const kNbtOff = "neighbour tables are off: rm_nbtable_enable comes first";

// what the feature keeps beside rm_context::Relay
static void nbtable_free(rm_context *c)
{
    rm_context::NbTable &nt = c->nt;
    nt.node.release(); nt.totals.release(); nt.bid.release();
}

void nbtable_release(rm_context *c) { relay_release(c, c->nt, nbtable_free); }

// on, and the statistics' tables it writes still there for the same node count
static int nbtable_have(const rm_context *c)
{
    RM_TRY(relay_have(c->nt, kNbtOff));
    RM_TRY(linkstats_have(c));
    if (c->lk.n != c->nt.n) return fail(RM_ERR_STATE, "internal: the watched-link statistics were made for another node count");
    return RM_OK;
}

static rm::NbTableDev nbtable_dev(const rm_context *c)
{
    const rm_context::NbTable &nt = c->nt;
    rm::NbTableDev f{};
    f.peer = c->lk.peer.p;
    f.table = c->lk.table.p;
    f.node = nt.node.p;
    f.totals = nt.totals.p;
    f.bid = nt.bid.p;
    f.n_nodes = nt.n;
    f.K = c->lk.K;
    f.p = nt.p;
    return f;
}

// a host pin array: no entry at or above the node count (negative entries: no pin), then in device memory (c->nt.stage.p)
static int nbtable_stage_pin(rm_context *c, const int32_t *pin)
{
    RM_TRY(relay_check_host_list(c->nt, pin, c->nt.n, "pin"));
    return relay_stage_list(c, c->nt, pin, c->nt.n);
}

static bool nbt_k_ok(int32_t K) { return K == 1 || K == 2 || K == 4 || K == 8; }

// what both host functions check
static int nbt_host_args(int32_t n_nodes, int32_t K, const int32_t *peer, const rm_link_stats *stats, const rm_nbtable_params *params, int64_t time_us,
                         const int32_t *pin)
{
    if (!params) return fail(RM_ERR_INVALID, "params is NULL");
    RM_TRY(rm_nbtable_validate(params));
    if (n_nodes < 0 || !nbt_k_ok(K) || time_us < 0 || (n_nodes > 0 && (!peer || !stats))) return fail(RM_ERR_INVALID, "bad arguments");
    for (int32_t d = 0; pin && d < n_nodes; ++d)
        if (pin[d] >= n_nodes) return fail(RM_ERR_INVALID, "an entry of the pin array is not below the node count");
    return RM_OK;
}

} // namespace rmh

extern "C" {

void rm_nbtable_defaults(rm_nbtable_params *p)
{
    if (!p) return;
    *p = rm_nbtable_params{};
    p->admit_rssi_dbm = -95.0;
    p->timeout_us = 60000000;
    p->min_heard = 4;
    p->evict_cost = 1024;
    p->require_delivered = 1;
}

int rm_nbtable_validate(const rm_nbtable_params *p)
{
    if (!p) return fail(RM_ERR_INVALID, "params is NULL");
    if (!rm::nbt_valid(*p))
        return fail(RM_ERR_INVALID, "bad rm_nbtable_params: admit_rssi_dbm finite, timeout_us 0 .. 2^62, min_heard 0 .. 2^31, evict_cost 0 or 128 .. "
                                    "2^32-1, require_delivered 0 or 1, reserved 0");
    return RM_OK;
}

int rm_nbtable_enable(rm_context *c, const rm_nbtable_params *p)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(rm_nbtable_validate(p));
    RM_TRY(graphs_refuse(c, "the extensions' tables are not set on it"));
    if (c->n < 1) return fail(RM_ERR_STATE, "no nodes: rm_nodes_upload comes first");
    RM_TRY(linkstats_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_off(c, c->nt, nbtable_free)); // (another enable: the counters anew)
    rm_context::NbTable &nt = c->nt;
    const size_t n = size_t(c->n);
    hipError_t e = nt.node.ensure(n);
    if (e == hipSuccess) e = nt.totals.ensure(1);
    if (e == hipSuccess) e = nt.bid.ensure(n);
    if (e == hipSuccess) {
        nt.p = *p;
        nt.n = c->n;
        e = rm::launch_nbtable_init(c->stream, nbtable_dev(c));
    }
    if (e != hipSuccess) {
        nbtable_release(c);
        return fail(RM_ERR_HIP, std::string("rm_nbtable_enable: ") + hipGetErrorString(e));
    }
    nt.on = true;
    return RM_OK;
}

int rm_nbtable_disable(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_HIP(hipSetDevice(c->device));
    return relay_off(c, c->nt, nbtable_free);
}

int rm_nbtable_enabled(const rm_context *c) { return (c && c->nt.on) ? 1 : 0; }

int rm_nbtable_get_params(const rm_context *c, rm_nbtable_params *out)
{
    if (!c || !out) return fail(RM_ERR_INVALID, "ctx or out is NULL");
    RM_TRY(relay_have(c->nt, kNbtOff));
    *out = c->nt.p;
    return RM_OK;
}

int rm_nbtable_reset(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(nbtable_have(c));
    RM_HIP(hipSetDevice(c->device));
    RM_HIP(rm::launch_nbtable_init(c->stream, nbtable_dev(c)));
    return RM_OK;
}

int rm_nbtable_update_device(rm_context *c, int32_t slot, int64_t time_us, const int32_t *dev_pin)
{
    if (!c || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(nbtable_have(c));
    rm::UcSlot d;
    int32_t P = 0;
    RM_TRY(relay_advance_begin(c, c->nt, kNbtOff, slot, nullptr, 0, &d, &P));
    CallProbe probe(c);
    RM_HIP(rm::launch_nbtable_update(c->stream, nbtable_dev(c), d, time_us, dev_pin));
    c->lk.host_stale = true; // (the peer rows changed on the device: rm_linkstats_peers_get reads them back)
    return RM_OK;
}

int rm_nbtable_update(rm_context *c, int32_t slot, int64_t time_us, const int32_t *pin)
{
    if (!c || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(nbtable_have(c));
    RM_TRY(relay_check_advance(c, c->nt, kNbtOff, slot, 0));
    if (pin) RM_TRY(nbtable_stage_pin(c, pin));
    return rm_nbtable_update_device(c, slot, time_us, pin ? c->nt.stage.p : nullptr);
}

int rm_nbtable_expire_device(rm_context *c, int64_t time_us, const int32_t *dev_pin)
{
    if (!c || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(nbtable_have(c));
    RM_HIP(hipSetDevice(c->device));
    CallProbe probe(c);
    RM_HIP(rm::launch_nbtable_expire(c->stream, nbtable_dev(c), time_us, dev_pin));
    c->lk.host_stale = true;
    return RM_OK;
}

int rm_nbtable_expire(rm_context *c, int64_t time_us, const int32_t *pin)
{
    if (!c || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(nbtable_have(c));
    if (pin) RM_TRY(nbtable_stage_pin(c, pin));
    return rm_nbtable_expire_device(c, time_us, pin ? c->nt.stage.p : nullptr);
}

int rm_nbtable_read(rm_context *c, const int32_t *nodes, int32_t n, rm_nbtable_node *out, rm_nbtable_totals *totals)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(relay_have(c->nt, kNbtOff));
    if (nodes || n != 0) RM_TRY(check_node_list(nodes, n, c->nt.n));
    RM_HIP(hipSetDevice(c->device));
    if (totals) RM_HIP(hipMemcpyAsync(totals, c->nt.totals.p, sizeof(rm_nbtable_totals), hipMemcpyDeviceToHost, c->stream));
    RM_TRY(rows_read(c, c->nt.h, c->nt.node.p, sizeof(rm_nbtable_node) / 8, c->nt.n, nodes, n, out, nullptr, nullptr));
    return RM_OK;
}

int rm_nbtable_device(rm_context *c, const rm_nbtable_node **dev_node, const rm_nbtable_totals **dev_totals)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(relay_have(c->nt, kNbtOff));
    if (dev_node) *dev_node = c->nt.node.p;
    if (dev_totals) *dev_totals = c->nt.totals.p;
    return RM_OK;
}

int rm_nbtable_from_result(const rm_host_result *r, const int32_t *src, const int64_t *start_us, int32_t n_nodes, int32_t K, int32_t *peer,
                           rm_link_stats *stats, const rm_nbtable_params *params, int64_t time_us, const int32_t *pin, rm_nbtable_node *node,
                           rm_nbtable_totals *totals)
{
    if (!r) return fail(RM_ERR_INVALID, "the result is NULL");
    RM_TRY(nbt_host_args(n_nodes, K, peer, stats, params, time_us, pin));
    const uint32_t n_pkt = r->n_packets;
    if (n_pkt > 0 && (!src || !start_us)) return fail(RM_ERR_INVALID, "src or start_us is NULL");
    const bool links = n_pkt > 0 && r->count > 0;
    if (links && (!r->pkt_offset || !r->dst || !r->verdict)) return fail(RM_ERR_INVALID, "the result lacks pkt_offset, dst or verdict");
    if (totals) totals->updates += 1;
    if (!links || n_nodes < 1) return RM_OK;
    const size_t Ks = size_t(K);
    auto rssi_of = [&](uint32_t p, uint32_t i) {
        return r->rssi ? r->rssi[i] : (r->pkt_rssi ? r->pkt_rssi[p] : std::numeric_limits<double>::quiet_NaN());
    };
    auto held = [&](int32_t d, int32_t s) {
        for (size_t k = 0; k < Ks; ++k)
            if (peer[size_t(d) * Ks + k] == s) return int(k);
        return -1;
    };
    auto for_links = [&](auto body) { // (p, i, s, d) of every link whose two ends are in the table
        for (uint32_t p = 0; p < n_pkt; ++p) {
            const uint32_t end = std::min(r->pkt_offset[p + 1], r->count);
            const int32_t s = src[p];
            if (!rm::nbt_in(n_nodes, s)) continue;
            for (uint32_t i = std::min(r->pkt_offset[p], end); i < end; ++i)
                if (rm::nbt_in(n_nodes, r->dst[i])) body(p, i, s, r->dst[i]);
        }
    };
    // (1) the bids, on the tables as they are
    std::vector<uint64_t> bid(size_t(n_nodes), 0);
    for_links([&](uint32_t p, uint32_t i, int32_t s, int32_t d) {
        if (s == d || held(d, s) >= 0) return;
        const double rssi = rssi_of(p, i);
        if (!rm::nbt_bids(*params, rssi, r->verdict[i] == uint8_t(RM_DELIVERED))) return;
        bid[size_t(d)] = std::max(bid[size_t(d)], rm::nbt_key(rssi, s));
    });
    // (2) a node's choice reads its own row only, which no other node's choice writes
    for (int32_t d = 0; d < n_nodes; ++d) {
        if (bid[size_t(d)] == 0) continue;
        int kind = 0;
        const int k = rm::nbt_settle(*params, n_nodes, K, d, peer + size_t(d) * Ks, stats + size_t(d) * Ks, time_us, pin ? pin[d] : -1, kind);
        if (k < 0) {
            bid[size_t(d)] = 0;
            if (node) node[d].refused += 1;
            if (totals) totals->refused += 1;
            continue;
        }
        peer[size_t(d) * Ks + size_t(k)] = rm::nbt_key_src(bid[size_t(d)]);
        rm::nbt_clear(stats[size_t(d) * Ks + size_t(k)]);
        if (node) node[d].admitted += 1;
        if (totals) totals->admitted += 1;
        if (kind == 1) {
            if (node) node[d].evicted_stale += 1;
            if (totals) totals->evicted_stale += 1;
        } else if (kind == 2) {
            if (node) node[d].evicted_poor += 1;
            if (totals) totals->evicted_poor += 1;
        }
    }
    // (3) the admitted peers' links of this slot, as the watched links' pass adds a link
    for_links([&](uint32_t p, uint32_t i, int32_t s, int32_t d) {
        if (bid[size_t(d)] == 0 || rm::nbt_key_src(bid[size_t(d)]) != s) return;
        const int k = held(d, s);
        if (k < 0) return;
        rm_link_stats &e = stats[size_t(d) * Ks + size_t(k)];
        e.heard += 1;
        if (r->verdict[i] == uint8_t(RM_DELIVERED)) e.delivered += 1;
        if (r->rssi || r->pkt_rssi) e.rssi_q8_sum = int64_t(uint64_t(e.rssi_q8_sum) + uint64_t(rm::linkstats_q8(rssi_of(p, i))));
        if (r->sinr) e.sinr_q8_sum = int64_t(uint64_t(e.sinr_q8_sum) + uint64_t(rm::linkstats_q8(r->sinr[i])));
        e.first_start_us = std::min(e.first_start_us, start_us[p]);
        e.last_start_us = std::max(e.last_start_us, start_us[p]);
    });
    return RM_OK;
}

int rm_nbtable_expire_tables(int32_t n_nodes, int32_t K, int32_t *peer, rm_link_stats *stats, const rm_nbtable_params *params, int64_t time_us,
                             const int32_t *pin, rm_nbtable_node *node, rm_nbtable_totals *totals)
{
    RM_TRY(nbt_host_args(n_nodes, K, peer, stats, params, time_us, pin));
    for (int32_t d = 0; d < n_nodes; ++d) {
        const int32_t pn = pin ? pin[d] : -1;
        const bool pinned = rm::nbt_in(n_nodes, pn);
        for (int32_t k = 0; k < K; ++k) {
            const size_t at = size_t(d) * size_t(K) + size_t(k);
            if (rm::nbt_empty(n_nodes, d, peer[at]) || (pinned && peer[at] == pn)) continue;
            if (!rm::nbt_stale(params->timeout_us, time_us, stats[at].last_start_us)) continue;
            peer[at] = -1;
            rm::nbt_clear(stats[at]);
            if (node) node[d].expired += 1;
            if (totals) totals->expired += 1;
        }
    }
    return RM_OK;
}

} // extern "C"
