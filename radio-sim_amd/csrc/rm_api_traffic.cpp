// rm_api_traffic.cpp -- C ABI: traffic schedules, periodic sources generated on the device (the kernels
// are rm_traffic.hip).
//
// The table belongs to the context: one rm_traffic_schedule per node index.  No evaluating call reads it; the generator turns it
// into the source lists those calls take.  Everything here sets, clears, reads and generates.
#include "rm_host.hpp"

using namespace rmh;

namespace rmh {

// off: the table forgotten (the buffers stay for the next rm_traffic_set)
static int traffic_off(rm_context *c)
{
    rm_context::Traffic &tf = c->tf;
    if (tf.n >= 0) RM_HIP(hipStreamSynchronize(c->stream)); // (a generate in flight still reads the table; pointers handed out end here)
    tf.on = false;
    tf.n = -1;
    return RM_OK;
}

int traffic_nodes_changed(rm_context *c)
{
    if (c->tf.n < 0 || c->tf.n == c->n) return RM_OK; // never set, or the same node count: the table stays
    return traffic_off(c);
}

void traffic_release(rm_context *c)
{
    rm_context::Traffic &tf = c->tf;
    tf.sched.release(); tf.d_win.release(); tf.d_unit_count.release(); tf.d_unit_packets.release();
    tf.h.release();
    for (int g = 0; g < 2; ++g) {
        if (tf.h_ev[g]) (void)hipEventDestroy(tf.h_ev[g]);
        if (tf.h_win[g]) (void)hipHostFree(tf.h_win[g]);
        tf.h_ev[g] = nullptr;
        tf.h_win[g] = nullptr;
    }
}

// the table for c->n nodes: every period 0
static int traffic_make(rm_context *c)
{
    rm_context::Traffic &tf = c->tf;
    if (tf.n == c->n && tf.sched.p) return RM_OK;
    RM_HIP(hipStreamSynchronize(c->stream));
    RM_HIP(tf.sched.ensure(size_t(std::max(c->n, 1))));
    RM_HIP(hipMemsetAsync(tf.sched.p, 0, size_t(std::max(c->n, 1)) * sizeof(rm_traffic_schedule), c->stream));
    tf.n = c->n;
    return RM_OK;
}

static int traffic_have(const rm_context *c)
{
    if (c->tf.n < 0) return fail(RM_ERR_STATE, "no traffic schedules: rm_traffic_set comes first");
    return RM_OK;
}

static int traffic_check_records(const rm_traffic_schedule *sched, int32_t n)
{
    for (int32_t k = 0; k < n; ++k)
        if (!rm::host_traffic_valid(sched[k]))
            return fail(RM_ERR_INVALID, "bad rm_traffic_schedule: period_us 0 with the other fields 0, or 1 <= period_us <= 2^40 with "
                                        "0 <= phase_us < period_us, 0 <= jitter_us <= period_us and reserved 0");
    return RM_OK;
}

static int traffic_check_windows(int32_t n_ticks, const int64_t *win_lo, const int64_t *win_hi, int32_t cap)
{
    if (!win_lo || !win_hi) return fail(RM_ERR_INVALID, "win_lo / win_hi is NULL");
    if (n_ticks < 1 || n_ticks > RM_MAX_BATCH) return fail(RM_ERR_INVALID, "n_ticks outside 1 .. RM_MAX_BATCH");
    if (cap < 1) return fail(RM_ERR_INVALID, "cap < 1");
    for (int32_t b = 0; b < n_ticks; ++b) {
        if (win_lo[b] < 0 || win_lo[b] > win_hi[b] || win_hi[b] > (int64_t(1) << 62))
            return fail(RM_ERR_INVALID, "a window needs 0 <= win_lo <= win_hi <= 2^62");
        if (b > 0 && win_hi[b - 1] > win_lo[b]) return fail(RM_ERR_INVALID, "the windows are in time order and disjoint");
    }
    if (int64_t(n_ticks) * int64_t(cap) > (int64_t(1) << 27)) return fail(RM_ERR_CAPACITY, "n_ticks * cap above 2^27");
    return RM_OK;
}

// a validated update: the table made if need be, then the whole table copied or the list scattered, on the context's stream
static int traffic_write(rm_context *c, const int32_t *nodes, int32_t n, const rm_traffic_schedule *sched)
{
    RM_TRY(traffic_make(c));
    rm_context::Traffic &tf = c->tf;
    if (!nodes) {
        if (n > 0) { // (waited for: the caller's array is free when this returns)
            RM_HIP(hipMemcpyAsync(tf.sched.p, sched, size_t(n) * sizeof(rm_traffic_schedule), hipMemcpyHostToDevice, c->stream));
            RM_HIP(hipStreamSynchronize(c->stream));
        }
    } else if (n > 0) { // a list: every entry staged with its node's final record (the last entry of a node wins)
        RM_TRY(rows_write<rm_traffic_schedule>(c, tf.h, tf.sched.p, tf.n, nodes, n, sched, rows_final(tf.h, nodes, n, tf.n)));
    }
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_traffic_validate(int32_t n_nodes, const int32_t *nodes, int32_t n, const rm_traffic_schedule *sched)
{
    if (n_nodes < 0 || n < 0 || (n > 0 && !sched)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(check_node_list(nodes, n, n_nodes));
    return traffic_check_records(sched, n);
}

int rm_traffic_set(rm_context *c, const int32_t *nodes, int32_t n, const rm_traffic_schedule *sched)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_TRY(graphs_refuse(c, "the extensions' tables are not set on it"));
    // the whole list is validated before anything changes
    RM_TRY(rm_traffic_validate(c->n, nodes, n, sched));
    RM_HIP(hipSetDevice(c->device));
    // a table this call makes and then fails to fill is forgotten again: `on` and the table the readers accept go together
    const bool had_table = c->tf.n >= 0;
    const int rc = traffic_write(c, nodes, n, sched);
    if (rc != RM_OK) {
        if (!had_table) c->tf.n = -1;
        return rc;
    }
    c->tf.on = true;
    return RM_OK;
}

int rm_traffic_get(rm_context *c, const int32_t *nodes, int32_t n, rm_traffic_schedule *out)
{
    if (!c || n < 0 || (n > 0 && !out)) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(traffic_have(c));
    RM_TRY(check_node_list(nodes, n, c->tf.n));
    RM_HIP(hipSetDevice(c->device));
    return rows_read(c, c->tf.h, c->tf.sched.p, sizeof(rm_traffic_schedule) / 8, c->tf.n, nodes, n, out, nullptr, nullptr);
}

int rm_traffic_clear(rm_context *c)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    RM_HIP(hipSetDevice(c->device));
    return traffic_off(c);
}

int rm_traffic_enabled(const rm_context *c) { return (c && c->tf.on) ? 1 : 0; }

int rm_traffic_device(rm_context *c, const rm_traffic_schedule **dev_sched)
{
    if (!c || !dev_sched) return fail(RM_ERR_INVALID, "ctx or dev_sched is NULL");
    RM_TRY(traffic_have(c));
    *dev_sched = c->tf.sched.p;
    return RM_OK;
}

int rm_traffic_generate_device(rm_context *c, uint64_t seed, int32_t n_ticks, const int64_t *win_lo, const int64_t *win_hi, int32_t cap,
                               int32_t *dev_src, int32_t *dev_count, rm_traffic_totals *dev_totals)
{
    if (!c || !dev_src || !dev_count) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(traffic_have(c));
    RM_TRY(traffic_check_windows(n_ticks, win_lo, win_hi, cap));
    RM_HIP(hipSetDevice(c->device));
    rm_context::Traffic &tf = c->tf;
    rm::TrafficGen g{};
    g.sched = tf.sched.p;
    g.n_nodes = tf.n;
    g.seed = seed;
    g.n_ticks = n_ticks;
    g.cap = cap;
    rm::traffic_geometry(tf.n, &g.units, &g.chunk);
    // scratch: made at the first generate, grown when a call needs more (the stream's earlier generates still use the old blocks)
    const size_t want_counts = size_t(g.units) * size_t(n_ticks);
    if (tf.d_win.n < size_t(2 * RM_MAX_BATCH) || tf.d_unit_count.n < want_counts || tf.d_unit_packets.n < size_t(g.units)) {
        RM_HIP(hipStreamSynchronize(c->stream));
        RM_HIP(tf.d_win.ensure(size_t(2 * RM_MAX_BATCH)));
        RM_HIP(tf.d_unit_count.ensure(want_counts));
        RM_HIP(tf.d_unit_packets.ensure(size_t(g.units)));
    }
    // the windows: through one of two pinned blocks, rewritten only after the copy out of it (two generates ago) has completed
    const int gen = tf.gen;
    tf.gen ^= 1;
    if (!tf.h_win[gen]) { // (the block and its event exist together or not at all)
        hipEvent_t ev = nullptr;
        RM_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&tf.h_win[gen]), size_t(2 * RM_MAX_BATCH) * sizeof(int64_t), hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipEventDestroy(ev);
            tf.h_win[gen] = nullptr;
            return fail(RM_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        }
        tf.h_ev[gen] = ev;
    } else {
        RM_HIP(hipEventSynchronize(tf.h_ev[gen]));
    }
    std::memcpy(tf.h_win[gen], win_lo, size_t(n_ticks) * sizeof(int64_t));
    std::memcpy(tf.h_win[gen] + n_ticks, win_hi, size_t(n_ticks) * sizeof(int64_t));
    RM_HIP(hipMemcpyAsync(tf.d_win.p, tf.h_win[gen], size_t(2 * n_ticks) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipEventRecord(tf.h_ev[gen], c->stream));
    g.win = tf.d_win.p;
    g.unit_count = tf.d_unit_count.p;
    g.unit_packets = tf.d_unit_packets.p;
    g.out_src = dev_src;
    g.out_count = dev_count;
    g.out_totals = dev_totals;
    CallProbe probe(c); // (rm_profile_kernels names the three kernels)
    RM_HIP(rm::launch_traffic_generate(c->stream, g));
    return RM_OK;
}

int rm_traffic_generate(rm_context *c, uint64_t seed, int32_t n_ticks, const int64_t *win_lo, const int64_t *win_hi, int32_t cap, int32_t *src,
                        int32_t *count, rm_traffic_totals *totals)
{
    if (!c || !src || !count) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(traffic_have(c));
    RM_TRY(traffic_check_windows(n_ticks, win_lo, win_hi, cap));
    RM_HIP(hipSetDevice(c->device));
    // the outputs' device block lives for this call only: rows, counts, totals
    const size_t rows = pad64(size_t(n_ticks) * size_t(cap) * 4), counts = pad64(size_t(n_ticks) * 4);
    char *d = nullptr;
    RM_HIP(hipMalloc(reinterpret_cast<void **>(&d), rows + counts + sizeof(rm_traffic_totals)));
    int32_t *d_src = reinterpret_cast<int32_t *>(d), *d_count = reinterpret_cast<int32_t *>(d + rows);
    rm_traffic_totals *d_totals = reinterpret_cast<rm_traffic_totals *>(d + rows + counts);
    int rc = rm_traffic_generate_device(c, seed, n_ticks, win_lo, win_hi, cap, d_src, d_count, d_totals);
    if (rc == RM_OK) {
        hipError_t e = hipMemcpyAsync(src, d_src, size_t(n_ticks) * size_t(cap) * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(count, d_count, size_t(n_ticks) * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && totals) e = hipMemcpyAsync(totals, d_totals, sizeof(rm_traffic_totals), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(RM_ERR_HIP, std::string("rm_traffic_generate: ") + hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

int rm_traffic_due(const rm_traffic_schedule *s, uint64_t seed, int32_t node, int64_t k, int64_t *due_us)
{
    if (!s || !due_us || node < 0 || k < 0 || !rm::host_traffic_valid(*s)) return RM_ERR_INVALID;
    if (s->period_us == 0) return 0;
    if (k > (int64_t(1) << 62) / s->period_us) return RM_ERR_INVALID;
    *due_us = rm::host_traffic_due(*s, seed, node, k);
    return 1;
}

} // extern "C"
