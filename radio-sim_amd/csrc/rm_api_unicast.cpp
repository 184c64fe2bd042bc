// rm_api_unicast.cpp -- C ABI: the unicast outcome query (the kernel is rm_unicast.hip).
//
// A read-only pass over the finished results of the last evaluating call.  Every check comes before the first launch; what is
// launched then is what any result reader may launch (a slot's compact arrays where the tick left them for later: materialize)
// and the query's one kernel.  The slots' descriptors (rm::UcSlot) are made from what the slots hold when the query comes -- as
// rm_batch_result_view makes its own -- so every evaluating form is covered, whichever launch sequence it took: a lone tick's goes
// to the kernel by value, a batch's through a pinned block into device memory, on the stream.
#include "rm_host.hpp"

#include <limits>

using namespace rmh;

namespace {

constexpr int64_t kUcMaxEntries = int64_t(1) << 27;

size_t uc_prefix_off() { return pad64(sizeof(rm::UcSlot) * RM_MAX_BATCH); }
size_t uc_desc_bytes() { return uc_prefix_off() + pad64(sizeof(uint32_t) * (RM_MAX_BATCH + 1)); }

} // namespace

namespace rmh {

// what every form refuses with RM_ERR_STATE: nothing launched, nothing changed
int uc_check_state(rm_context *c)
{
    RM_TRY(graphs_refuse(c, "the query's pass is not part of them"));
    if (c->uc.slots <= 0 || !c->have_result) return fail(RM_ERR_STATE, "no evaluated result yet");
    if (part_spatial(c) || part_count(c) != c->n)
        return fail(RM_ERR_STATE, "a context with a receiver partition does not hold the other ranks' links: RM_UC_UNHEARD would be a lie");
    if (c->uc.gathered) return fail(RM_ERR_STATE, "the last evaluating call was a gathered / rm_dist_* / rm_group_* form");
    for (int b = 0; b < c->uc.slots; ++b) {
        const TickSlot *ts = slot_of(c, b);
        if (!ts || !ts->have_result) return fail(RM_ERR_STATE, "no evaluated result in a slot of the last call");
        if (ts->draws_pending) return fail(RM_ERR_STATE, "a slot's verdicts wait for rm_tick_finish_draws");
    }
    return RM_OK;
}

} // namespace rmh

namespace {

int uc_check_out(const rm_unicast_out *out)
{
    if (!out) return fail(RM_ERR_INVALID, "the output table is NULL");
    return RM_OK;
}

} // namespace

namespace rmh {

// the slot's compact arrays (written now if the tick left them for later), described for the kernel
int uc_describe(rm_context *c, TickSlot &ts, rm::UcSlot *d)
{
    RM_TRY(materialize(c, ts));
    const rm::TickDev &t = ts.last;
    const int n_new = std::max(ts.last_n_new, 0);
    *d = rm::UcSlot{};
    d->n_new = n_new;
    d->recs = (t.tx && n_new > 0) ? t.tx + t.first_new : nullptr;
    d->pkt_offset = (n_new > 0 && part_count(c) > 0) ? ts.d_slot_off.p + t.shift : nullptr; // (as copy_out reads them)
    d->dst = ts.d_out_dst.p;
    d->verdict = ts.d_out_verdict.p;
    d->rssi = ts.d_out_rssi.p;
    d->sinr = t.out_sinr; // nullptr without the SINR extension
    d->out_count = t.out_count;
    d->stage_count = t.stage_count;
    return RM_OK;
}

// The descriptors of all slots of the last call for the kernel: one slot goes by value (*lone); several go to device memory --
// *dev_slots -- with the prefix of a slots-form query behind them (*dev_prefix; prefix: n_prefix + 1 words, or nullptr).  all: the
// query can reach a slot behind slot 0.
int uc_slots(rm_context *c, bool all, const uint32_t *prefix, int n_prefix, rm::UcSlot *lone, const rm::UcSlot **dev_slots, const uint32_t **dev_prefix)
{
    rm_context::Unicast &u = c->uc;
    *dev_slots = nullptr;
    *dev_prefix = nullptr;
    RM_TRY(uc_describe(c, *c, lone));
    if (!all || u.slots == 1) return RM_OK;
    const int g = u.gen;
    u.gen ^= 1;
    if (!u.h_desc[g]) {
        RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&u.h_desc[g]), uc_desc_bytes(), hipHostMallocDefault));
        RM_HIP(hipEventCreateWithFlags(&u.h_ev[g], hipEventDisableTiming));
    } else {
        RM_HIP(hipEventSynchronize(u.h_ev[g])); // (the copy out of this block, two queries ago)
    }
    RM_HIP(u.d_desc.ensure(uc_desc_bytes()));
    rm::UcSlot *h = reinterpret_cast<rm::UcSlot *>(u.h_desc[g]);
    h[0] = *lone;
    for (int b = 1; b < u.slots; ++b) RM_TRY(uc_describe(c, *slot_of(c, b), h + b));
    size_t bytes = sizeof(rm::UcSlot) * size_t(u.slots);
    if (prefix) {
        std::memcpy(u.h_desc[g] + uc_prefix_off(), prefix, sizeof(uint32_t) * (size_t(n_prefix) + 1));
        bytes = uc_prefix_off() + sizeof(uint32_t) * (size_t(n_prefix) + 1);
        *dev_prefix = reinterpret_cast<const uint32_t *>(u.d_desc.p + uc_prefix_off());
    }
    RM_HIP(hipMemcpyAsync(u.d_desc.p, u.h_desc[g], bytes, hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipEventRecord(u.h_ev[g], c->stream));
    *dev_slots = reinterpret_cast<const rm::UcSlot *>(u.d_desc.p);
    return RM_OK;
}

} // namespace rmh

namespace {

// the slots form's checks behind the state: the prefix of n_pkt (n_slots + 1 words) and the number of entries
int uc_check_slots(rm_context *c, int32_t n_slots, const int32_t *n_pkt, std::vector<uint32_t> &prefix, int64_t *total)
{
    if (n_slots < 1 || n_slots > c->uc.slots) return fail(RM_ERR_INVALID, "n_slots outside 1 .. the slots of the last evaluating call");
    prefix.assign(size_t(n_slots) + 1, 0u);
    int64_t n = 0;
    for (int b = 0; b < n_slots; ++b) {
        if (n_pkt[b] < 0) return fail(RM_ERR_INVALID, "a negative n_pkt");
        n += n_pkt[b];
        if (n > kUcMaxEntries) return fail(RM_ERR_CAPACITY, "more than 2^27 query entries");
        prefix[size_t(b) + 1] = uint32_t(n);
    }
    *total = n;
    return RM_OK;
}

int uc_check_want_host(const rm_context *c, const int32_t *want, int64_t n)
{
    for (int64_t e = 0; e < n; ++e)
        if (want[e] >= c->n) return fail(RM_ERR_INVALID, "a wanted node of a host list is not below the node count");
    return RM_OK;
}

// the host forms' device scratch for n entries: three lists in, the five outputs
struct UcIo {
    int32_t *slot, *pkt, *want;
    rm_unicast_out out;
};

int uc_io(rm_context *c, int64_t n, UcIo *io)
{
    const size_t k = size_t(n);
    size_t o = 0;
    const size_t o_rssi = o; o += pad64(k * 8);
    const size_t o_sinr = o; o += pad64(k * 8);
    const size_t o_link = o; o += pad64(k * 4);
    const size_t o_reply = o; o += pad64(k * 4);
    const size_t o_slot = o; o += pad64(k * 4);
    const size_t o_pkt = o; o += pad64(k * 4);
    const size_t o_want = o; o += pad64(k * 4);
    const size_t o_status = o; o += pad64(k);
    RM_HIP(c->uc.d_io.ensure(std::max<size_t>(o, 64)));
    char *p = c->uc.d_io.p;
    io->out.rssi = reinterpret_cast<double *>(p + o_rssi);
    io->out.sinr = reinterpret_cast<double *>(p + o_sinr);
    io->out.link = reinterpret_cast<int32_t *>(p + o_link);
    io->out.reply_src = reinterpret_cast<int32_t *>(p + o_reply);
    io->out.status = reinterpret_cast<uint8_t *>(p + o_status);
    io->slot = reinterpret_cast<int32_t *>(p + o_slot);
    io->pkt = reinterpret_cast<int32_t *>(p + o_pkt);
    io->want = reinterpret_cast<int32_t *>(p + o_want);
    return RM_OK;
}

// only what the caller asked for is computed and copied
rm_unicast_out uc_asked(const rm_unicast_out &dev, const rm_unicast_out &host)
{
    rm_unicast_out o = dev;
    if (!host.status) o.status = nullptr;
    if (!host.link) o.link = nullptr;
    if (!host.rssi) o.rssi = nullptr;
    if (!host.sinr) o.sinr = nullptr;
    if (!host.reply_src) o.reply_src = nullptr;
    return o;
}

int uc_copy_back(rm_context *c, int64_t n, const rm_unicast_out &dev, const rm_unicast_out &host)
{
    const size_t k = size_t(n);
    hipStream_t s = c->stream;
    if (host.status) RM_HIP(hipMemcpyAsync(host.status, dev.status, k, hipMemcpyDeviceToHost, s));
    if (host.link) RM_HIP(hipMemcpyAsync(host.link, dev.link, k * 4, hipMemcpyDeviceToHost, s));
    if (host.rssi) RM_HIP(hipMemcpyAsync(host.rssi, dev.rssi, k * 8, hipMemcpyDeviceToHost, s));
    if (host.sinr) RM_HIP(hipMemcpyAsync(host.sinr, dev.sinr, k * 8, hipMemcpyDeviceToHost, s));
    if (host.reply_src) RM_HIP(hipMemcpyAsync(host.reply_src, dev.reply_src, k * 4, hipMemcpyDeviceToHost, s));
    RM_HIP(hipStreamSynchronize(s));
    return RM_OK;
}

} // namespace

extern "C" {

int rm_unicast_query_device(rm_context *c, int32_t n_slots, const int32_t *n_pkt, const int32_t *dev_want, const rm_unicast_out *dev_out)
{
    if (!c || !n_pkt || n_slots < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(uc_check_out(dev_out));
    RM_TRY(uc_check_state(c));
    static thread_local std::vector<uint32_t> prefix;
    int64_t n = 0;
    RM_TRY(uc_check_slots(c, n_slots, n_pkt, prefix, &n));
    if (n > 0 && !dev_want) return fail(RM_ERR_INVALID, "the list of wanted nodes is NULL");
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    rm::UcSlot lone;
    const rm::UcSlot *dev_slots = nullptr;
    const uint32_t *dev_prefix = nullptr;
    RM_TRY(uc_slots(c, n_slots > 1, prefix.data(), n_slots, &lone, &dev_slots, &dev_prefix));
    RM_HIP(rm::launch_unicast_slots(c->stream, dev_slots, lone, n_slots, dev_prefix, n, c->n, dev_want, *dev_out));
    return RM_OK;
}

int rm_unicast_query(rm_context *c, int32_t n_slots, const int32_t *n_pkt, const int32_t *want, const rm_unicast_out *out)
{
    if (!c || !n_pkt || n_slots < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(uc_check_out(out));
    RM_TRY(uc_check_state(c));
    static thread_local std::vector<uint32_t> prefix;
    int64_t n = 0;
    RM_TRY(uc_check_slots(c, n_slots, n_pkt, prefix, &n));
    if (n > 0 && !want) return fail(RM_ERR_INVALID, "the list of wanted nodes is NULL");
    RM_TRY(uc_check_want_host(c, want, n));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    UcIo io;
    RM_TRY(uc_io(c, n, &io));
    RM_HIP(hipMemcpyAsync(io.want, want, size_t(n) * 4, hipMemcpyHostToDevice, c->stream));
    const rm_unicast_out dev = uc_asked(io.out, *out);
    RM_TRY(rm_unicast_query_device(c, n_slots, n_pkt, io.want, &dev));
    return uc_copy_back(c, n, dev, *out);
}

int rm_unicast_query_at_device(rm_context *c, int64_t n, const int32_t *dev_slot, const int32_t *dev_pkt, const int32_t *dev_want,
                               const rm_unicast_out *dev_out)
{
    if (!c || n < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(uc_check_out(dev_out));
    if (n > 0 && (!dev_slot || !dev_pkt || !dev_want)) return fail(RM_ERR_INVALID, "a list of the query is NULL");
    RM_TRY(uc_check_state(c));
    if (n > kUcMaxEntries) return fail(RM_ERR_CAPACITY, "more than 2^27 query entries");
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    rm::UcSlot lone;
    const rm::UcSlot *dev_slots = nullptr;
    const uint32_t *dev_prefix = nullptr;
    RM_TRY(uc_slots(c, true, nullptr, 0, &lone, &dev_slots, &dev_prefix));
    RM_HIP(rm::launch_unicast_at(c->stream, dev_slots, lone, c->uc.slots, n, c->n, dev_slot, dev_pkt, dev_want, *dev_out));
    return RM_OK;
}

int rm_unicast_query_at(rm_context *c, int64_t n, const int32_t *slot, const int32_t *pkt, const int32_t *want, const rm_unicast_out *out)
{
    if (!c || n < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(uc_check_out(out));
    if (n > 0 && (!slot || !pkt || !want)) return fail(RM_ERR_INVALID, "a list of the query is NULL");
    RM_TRY(uc_check_state(c));
    if (n > kUcMaxEntries) return fail(RM_ERR_CAPACITY, "more than 2^27 query entries");
    RM_TRY(uc_check_want_host(c, want, n));
    if (n == 0) return RM_OK;
    RM_HIP(hipSetDevice(c->device));
    UcIo io;
    RM_TRY(uc_io(c, n, &io));
    RM_HIP(hipMemcpyAsync(io.slot, slot, size_t(n) * 4, hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipMemcpyAsync(io.pkt, pkt, size_t(n) * 4, hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipMemcpyAsync(io.want, want, size_t(n) * 4, hipMemcpyHostToDevice, c->stream));
    const rm_unicast_out dev = uc_asked(io.out, *out);
    RM_TRY(rm_unicast_query_at_device(c, n, io.slot, io.pkt, io.want, &dev));
    return uc_copy_back(c, n, dev, *out);
}

// the same answer from one tick's host result: no device, no context
int rm_unicast_from_result(const rm_host_result *r, const int32_t *src, int32_t n_nodes, const int32_t *want, const rm_unicast_out *out)
{
    if (!r || !out || n_nodes < 0) return fail(RM_ERR_INVALID, "bad arguments");
    const uint32_t n = r->n_packets;
    if (n > 0 && !want) return fail(RM_ERR_INVALID, "the list of wanted nodes is NULL");
    for (uint32_t p = 0; p < n; ++p)
        if (want[p] >= n_nodes) return fail(RM_ERR_INVALID, "a wanted node is not below the node count");
    if (n > 0 && r->count > 0 && (!r->pkt_offset || !r->dst || !r->verdict)) return fail(RM_ERR_INVALID, "the result lacks pkt_offset, dst or verdict");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t p = 0; p < n; ++p) {
        const int32_t w = want[p];
        int status = RM_UC_NONE;
        int32_t link = -1, reply = -1;
        double rssi = nan, sinr = nan;
        if (w >= 0) {
            if (src && (src[p] < 0 || src[p] >= n_nodes)) {
                status = RM_UC_NOT_SENT;
            } else {
                status = RM_UC_UNHEARD;
                if (r->pkt_offset && r->dst && r->verdict) {
                    const uint32_t end = std::min(r->pkt_offset[p + 1], r->count);
                    const uint32_t first = std::min(r->pkt_offset[p], end);
                    const int32_t *at = std::lower_bound(r->dst + first, r->dst + end, w);
                    if (at != r->dst + end && *at == w) {
                        const uint32_t i = uint32_t(at - r->dst);
                        link = int32_t(i);
                        const bool delivered = r->verdict[i] == uint8_t(RM_DELIVERED);
                        status = delivered ? RM_UC_DELIVERED : RM_UC_INTERFERED;
                        if (delivered) reply = w;
                        if (r->rssi) rssi = r->rssi[i];
                        else if (r->pkt_rssi) rssi = r->pkt_rssi[p];
                        if (r->sinr) sinr = r->sinr[i];
                    }
                }
            }
        }
        if (out->status) out->status[p] = uint8_t(status);
        if (out->link) out->link[p] = link;
        if (out->rssi) out->rssi[p] = rssi;
        if (out->sinr) out->sinr[p] = sinr;
        if (out->reply_src) out->reply_src[p] = reply;
    }
    return RM_OK;
}

} // extern "C"
