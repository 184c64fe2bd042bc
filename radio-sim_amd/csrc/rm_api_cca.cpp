// rm_api_cca.cpp -- C ABI: the carrier-sense gated tick (rm_tick_run_sources_cca*; k_cca_gate in rm_energy.hip)
// and the gated batch (rm_batch_run_sources_cca*; E7; rm_ccabatch.hip).
//
// One call: the candidates are sensed on the device over the on-air window as it is when the tick begins (E5 at cca_time_us, each on
// its own channel), the ones that find the channel busy -- or are on the air themselves -- become padding entries of a source list
// the context owns, and the unchanged SINR lone tick runs over that list.  Everything is ordered on the context's stream; the host
// learns nothing in between.
#include "rm_host.hpp"

using namespace rmh;

namespace {

// one gated tick's times, lone or of a batch: the sample lies between the tick's begin and its frames' start
int cca_times_check(int64_t t_begin_us, int64_t start_us, int64_t air_us, int64_t cca_time_us)
{
    if (cca_time_us < t_begin_us)
        return fail(RM_ERR_INVALID, "cca_time_us is earlier than t_begin_us: frames that had left the air by then are gone");
    if (cca_time_us > start_us)
        return fail(RM_ERR_INVALID, "cca_time_us is later than start_us: the sample would have to see the frames of its own tick");
    if (air_us > int64_t(UINT32_MAX)) return fail(RM_ERR_INVALID, "a frame of the SINR medium has to be shorter than 2^32 us");
    return RM_OK;
}

} // namespace

namespace rmh {

// the arguments of a gated batch as such: the caller's lists
int cca_batch_check_lists(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                          const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us)
{
    if (!c || n_ticks < 1 || n_ticks > RM_MAX_BATCH || !t_begin_us || !t_end_us || !src || !n_src || !start_us || !air_us || !cca_time_us)
        return fail(RM_ERR_INVALID, "bad arguments");
    size_t total = 0;
    for (int b = 0; b < n_ticks; ++b) {
        if (n_src[b] < 0 || (n_src[b] > 0 && !src[b]) || air_us[b] < 0) return fail(RM_ERR_INVALID, "bad arguments");
        total += size_t(n_src[b]);
    }
    if (total > size_t(1) << 30) return fail(RM_ERR_CAPACITY, "more than 2^30 candidates in one gated batch");
    return RM_OK;
}

// ... and the ticks with the number of candidates each of them senses (n_per: the lists' lengths, or the expanded lists' of a CSMA-CA batch)
int cca_batch_check_ticks(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int32_t *n_per, const int64_t *start_us,
                          const int64_t *air_us, const int64_t *cca_time_us)
{
    const int32_t *const n_src = n_per;
    int64_t clock = INT64_MIN; // the latest t_begin of the ticks before: the window's clock as lone gated ticks would have moved it
    for (int b = 0; b < n_ticks; ++b) {
        if (b == 0) RM_TRY(energy_check(c, cca_time_us[0], n_src[0], true));
        RM_TRY(cca_times_check(t_begin_us[b], start_us[b], air_us[b], cca_time_us[b]));
        if (cca_time_us[b] < clock)
            return fail(RM_ERR_INVALID, "cca_time_us is earlier than the t_begin_us of an earlier tick of the batch");
        clock = std::max(clock, t_begin_us[b]);
    }
    if (overlap_wanted(c, n_ticks, t_begin_us, n_src, start_us, air_us)) { // (batch_run_overlap's refusals that do not need a plan)
        if (maybe_draws(c))
            return fail(RM_ERR_STATE, "the SINR medium carries frames that outlive their tick and its links can draw: run overlapping "
                                      "ticks one at a time");
        for (int b = 0; b + 1 < n_ticks; ++b)
            if (t_begin_us[b + 1] < t_begin_us[b]) return fail(RM_ERR_STATE, "overlapping SINR ticks of a batch have to be in time order");
        RM_TRY(prepare_nodes(c));
        if (!c->rx_sorted || c->n_rx <= 0)
            return fail(RM_ERR_STATE, "the SINR medium carries frames that outlive their tick into the next one: run overlapping ticks one "
                                      "at a time (the batched form needs the spatially sorted receiver table)");
        // (batch_eligible, as far as it follows from the arguments and the table: the tick's frame count and the fp32 frame; what
        // is left -- the sweep's plan of a tick -- only batch_run_overlap itself can tell, after the gate)
        bool fits = c->f32_slack <= 0.05;
        for (int b = 0; b < n_ticks; ++b) fits = fits && n_src[b] <= rm::kFusedScanMax;
        if (!fits)
            return fail(RM_ERR_STATE, "the SINR medium carries frames that outlive their tick into the next one: run overlapping ticks one "
                                      "at a time (the batched form takes non-empty ticks of at most 8192 frames over an fp32 frame)");
    }
    return RM_OK;
}

// the pinned, host-mapped block of the gated batches: CcaTick[RM_MAX_BATCH], the words the device hands back (CcaBatchDev::h_info), then
// `extra` bytes the call uploads from (free: every call waits for its own scan)
int cca_desc_block(rm_context *c, size_t extra, rm::CcaTick **h_ticks, uint32_t **h_info, char **h_extra)
{
    rm_context::Energy::Batch &k = c->ed.cb;
    const size_t desc_bytes = pad64(sizeof(rm::CcaTick) * RM_MAX_BATCH);
    if (!k.h_desc || k.h_desc_extra < extra) {
        uint32_t sticky = 0u;
        if (k.h_desc) {
            RM_HIP(hipStreamSynchronize(c->stream));
            sticky = reinterpret_cast<uint32_t *>(k.h_desc + desc_bytes)[1];
            RM_HIP(hipHostFree(k.h_desc));
            k.h_desc = nullptr;
        }
        const size_t want = pad64(extra + extra / 2);
        RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&k.h_desc), desc_bytes + 64 + want, hipHostMallocMapped));
        std::memset(k.h_desc, 0, desc_bytes + 64);
        reinterpret_cast<uint32_t *>(k.h_desc + desc_bytes)[1] = sticky;
        k.h_desc_extra = want;
    }
    *h_ticks = reinterpret_cast<rm::CcaTick *>(k.h_desc);
    *h_info = reinterpret_cast<uint32_t *>(k.h_desc + desc_bytes);
    if (h_extra) *h_extra = k.h_desc + desc_bytes + 64;
    return RM_OK;
}

// The gate's buffers for n_cand candidates over n_ticks ticks (tick b: n_per[b] of them, list src[b]) and the window as it is now, the
// descriptors in the pinned block, the gated lists' places (gated_v) -- everything of CcaBatchDev but the pair list, which is sized
// after the counting pass.  The CSMA-CA batch takes the same with its expanded slots for candidates.
int cca_batch_dev(rm_context *c, size_t n_cand, int32_t n_ticks, const int32_t *const *src, const int32_t *n_per, const int64_t *start_us,
                  const int64_t *air_us, const int64_t *cca_time_us, size_t extra, rm::CcaBatchDev *out, bool *use_grid, rm::CcaTick **h_ticks_out,
                  const int32_t **gated_v, char **h_extra)
{
    rm_context::Energy &e = c->ed;
    rm_context::Energy::Batch &k = e.cb;
    RM_TRY(prepare_nodes(c));
    if (c->n_rx != c->n) return fail(RM_ERR_STATE, "internal: the receiver table does not hold every node");
    const size_t n_win = c->air_tail - c->air_head;
    const size_t n_frames = n_win + n_cand;
    if (n_frames > size_t(INT32_MAX) / 2) return fail(RM_ERR_CAPACITY, "on-air window too large");
    const bool grid = *use_grid = n_frames >= size_t(rm::kEdSmallWindow);
    rm::CcaTick *h_ticks = nullptr;
    uint32_t *h_info = nullptr;
    RM_TRY(cca_desc_block(c, extra, &h_ticks, &h_info, h_extra));
    RM_HIP(e.gated.ensure(n_cand));
    RM_HIP(k.ticks.ensure(RM_MAX_BATCH));
    RM_HIP(k.scr.ensure(n_cand));
    RM_HIP(k.cand.ensure(n_cand));
    RM_HIP(k.fr_tick.ensure(n_frames));
    RM_HIP(k.self_next.ensure(n_frames));
    RM_HIP(k.cnt.ensure(2 + size_t(rm::kEdCells)));
    RM_HIP(k.every_f.ensure(n_frames));
    RM_HIP(k.every_m.ensure(n_frames));
    RM_HIP(k.every_t.ensure(n_frames));
    if (grid) {
        RM_HIP(k.bucket_f.ensure(size_t(rm::kEdCells) * rm::kCbK));
        RM_HIP(k.bucket_m.ensure(size_t(rm::kEdCells) * rm::kCbK));
        RM_HIP(k.bucket_t.ensure(size_t(rm::kEdCells) * rm::kCbK));
    }
    RM_HIP(k.pair_cnt.ensure(n_cand));
    RM_HIP(k.pair_off.ensure(n_cand + 1));
    RM_HIP(k.pair_fill.ensure(n_cand));
    RM_HIP(k.pair_base.ensure((n_cand + 1023) / 1024));
    RM_HIP(k.base.ensure(n_cand));
    RM_HIP(k.base_flags.ensure(n_cand));
    RM_HIP(k.kept.ensure(n_cand));
    // the nodes' chains of own frames: the array and the stamp of the lone tick by scan and of the batch (rm_api_airbatch.cpp)
    if (c->d_self_slot.n < size_t(std::max(c->n, 1))) {
        RM_HIP(c->d_self_slot.ensure(size_t(std::max(c->n, 1))));
        RM_HIP(hipMemsetAsync(c->d_self_slot.p, 0, c->d_self_slot.n * sizeof(unsigned long long), c->stream));
    }
    if (++c->air.stamp == 0u) {
        c->air.stamp = 1u;
        RM_HIP(hipMemsetAsync(c->d_self_slot.p, 0, c->d_self_slot.n * sizeof(unsigned long long), c->stream));
    }
    rm::CcaBatchDev &cb = *out;
    cb = rm::CcaBatchDev{};
    cb.win = c->d_air.p + c->air_head;
    cb.scr = k.scr.p;
    cb.ticks = k.ticks.p;
    cb.n_win = int(n_win);
    cb.n_cand = int(n_cand);
    cb.n_ticks = n_ticks;
    cb.t_lo = INT64_MAX;
    cb.t_hi = INT64_MIN;
    int first = 0;
    for (int b = 0; b < n_ticks; ++b) {
        h_ticks[b] = rm::CcaTick{src[b], start_us[b], air_us[b], cca_time_us[b], first, n_per[b]};
        gated_v[size_t(b)] = e.gated.p + first;
        first += n_per[b];
        if (n_per[b] > 0) {
            cb.t_lo = std::min(cb.t_lo, cca_time_us[b]);
            cb.t_hi = std::max(cb.t_hi, cca_time_us[b]);
        }
    }
    cb.cand = k.cand.p;
    cb.fr_tick = k.fr_tick.p;
    cb.cnt = k.cnt.p;
    cb.bucket_f = k.bucket_f.p;
    cb.bucket_m = k.bucket_m.p;
    cb.bucket_t = k.bucket_t.p;
    cb.every_f = k.every_f.p;
    cb.every_m = k.every_m.p;
    cb.every_t = k.every_t.p;
    cb.self_slot = c->d_self_slot.p;
    cb.self_next = k.self_next.p;
    cb.stamp = c->air.stamp;
    cb.half = std::max(float(c->coord_bound), 1e-20f);
    cb.inv = float(rm::kEdG) / (2.0f * cb.half);
    cb.pair_cnt = k.pair_cnt.p;
    cb.pair_off = k.pair_off.p;
    cb.pair_fill = k.pair_fill.p;
    cb.pair_base = k.pair_base.p;
    cb.base = k.base.p;
    cb.base_flags = k.base_flags.p;
    cb.kept = k.kept.p;
    cb.h_info = h_info;
    *h_ticks_out = h_ticks;
    return RM_OK;
}

} // namespace rmh

namespace {

// what both forms refuse, before anything is launched and with nothing changed
int cca_check(rm_context *c, int64_t t_begin_us, const int32_t *src, int32_t n, int64_t start_us, int64_t air_us, int64_t cca_time_us)
{
    if (!c || n < 0 || (n > 0 && !src) || air_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(energy_check(c, cca_time_us, n, true));
    return cca_times_check(t_begin_us, start_us, air_us, cca_time_us);
}

// src / flags / energy: device-visible memory (flags and energy may be NULL)
int cca_tick(rm_context *c, int64_t t_begin_us, int64_t t_end_us, const int32_t *src, int32_t n, int64_t start_us, int64_t air_us,
             int64_t cca_time_us, double cca_threshold, uint8_t *flags, double *energy)
{
    RM_HIP(hipSetDevice(c->device));
    c->t_begin = t_begin_us;
    c->t_end = t_end_us;
    if (n == 0) return air_tick_device(c, t_begin_us, src, nullptr, 0, start_us, air_us, start_us + air_us, false);
    // The window as the tick will find it: expired for t_begin and with room for the new records (air_tick_device does both again
    // and finds nothing left to do), so that the gate reads [air_head, air_tail) of the buffer the tick appends to.
    RM_TRY(air_window_expire(c, t_begin_us));
    RM_TRY(air_window_reserve(c, size_t(n)));
    RM_HIP(c->ed.gated.ensure(size_t(n)));
    RM_TRY(energy_launch(c, cca_time_us, src, n, RM_CHANNEL_OWN, cca_threshold, energy, flags, c->ed.gated.p));
    return air_tick_device(c, t_begin_us, c->ed.gated.p, nullptr, n, start_us, air_us, start_us + air_us, false);
}

// ---- the gated batch (E7) --------------------------------------------------------------------------------------------------------
// what both forms refuse, before anything is launched and with nothing changed: the lone gated tick's refusals for every tick, and
// what rm_batch_run_sources_device refuses for the same arguments before it touches the window
int cca_batch_check(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                    const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us)
{
    RM_TRY(cca_batch_check_lists(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us));
    return cca_batch_check_ticks(c, n_ticks, t_begin_us, n_src, start_us, air_us, cca_time_us);
}

// src[b] / flags / energy: device-visible memory (flags and energy: flat over the ticks, may be NULL)
int cca_batch(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src, const int32_t *n_src,
              const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us, double cca_threshold, uint8_t *flags, double *energy)
{
    RM_HIP(hipSetDevice(c->device));
    size_t n_cand = 0;
    for (int b = 0; b < n_ticks; ++b) n_cand += size_t(n_src[b]);
    rm_context::Energy &e = c->ed;
    rm_context::Energy::Batch &k = e.cb;
    static thread_local std::vector<const int32_t *> gated_v;
    gated_v.assign(size_t(n_ticks), nullptr);
    if (n_cand > 0) {
        // the window as the batch will find it (batch_run does both again and finds nothing left to do)
        RM_TRY(air_window_expire(c, t_begin_us[0]));
        RM_TRY(air_window_reserve(c, n_cand));
        rm::CcaBatchDev cb{};
        bool grid = false;
        rm::CcaTick *h_ticks = nullptr;
        RM_TRY(cca_batch_dev(c, n_cand, n_ticks, src, n_src, start_us, air_us, cca_time_us, 0, &cb, &grid, &h_ticks, gated_v.data(), nullptr));
        uint32_t *const h_info = cb.h_info;
        rm::ModelDev m = model_dev(c);
        if (c->f32_slack > 0.05) m.shadow_tbl = nullptr; // (as the query: the link-hash table goes with the fp32 filter of a small frame)
        {
            CallProbe probe(c); // (rm_profile_kernels names the kernels that ran)
            sample_stage(probe.smp, RM_STAGE_SINR);
            h_info[0] = 0u;
            RM_HIP(rm::launch_ccab_count(c->stream, nodes_dev(c), m, cb, h_ticks, k.ticks.p, grid));
            // The one place where the host has to know a number of the device's: the pairs of all candidates, counted, not guessed.
            RM_HIP(hipStreamSynchronize(c->stream));
            if (h_info[1] != 0u) return fail(RM_ERR_HIP, "internal: a candidate's pairs outgrew their counted segment in an earlier gated batch");
            if (h_info[0] == 0xFFFFFFFFu) return fail(RM_ERR_CAPACITY, "more than 2^32 (candidate, frame) pairs in one gated batch: use smaller batches");
            const size_t n_pairs = std::max<size_t>(h_info[0], 1);
            RM_HIP(k.pair_slot.ensure(n_pairs));
            RM_HIP(k.pair_term.ensure(n_pairs));
            cb.pair_slot = k.pair_slot.p;
            cb.pair_term = k.pair_term.p;
            RM_HIP(rm::launch_ccab_resolve(c->stream, nodes_dev(c), m, cb, grid, cca_threshold, e.gated.p, energy, flags));
        }
    }
    // the unchanged batch over the gated lists (a tick without candidates keeps its NULL list)
    const int rc = batch_run(c, n_ticks, t_begin_us, t_end_us, gated_v.data(), nullptr, n_src, start_us, air_us);
    ev_batch_ran(c, rc, n_ticks, true);
    return rc;
}

} // namespace

extern "C" {

int rm_batch_run_sources_cca_device(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *dev_src,
                                    const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                                    double cca_threshold_dbm, uint8_t *dev_cca_flags, double *dev_cca_energy_dbm)
{
    RM_TRY(cca_batch_check(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us));
    return cca_batch(c, n_ticks, t_begin_us, t_end_us, dev_src, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, dev_cca_flags,
                     dev_cca_energy_dbm);
}

int rm_batch_run_sources_cca(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                             const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us,
                             double cca_threshold_dbm, uint8_t *cca_flags, double *cca_energy_dbm)
{
    RM_TRY(cca_batch_check(c, n_ticks, t_begin_us, t_end_us, src, n_src, start_us, air_us, cca_time_us));
    size_t total = 0;
    for (int b = 0; b < n_ticks; ++b) {
        for (int32_t k = 0; k < n_src[b]; ++k)
            if (src[b][k] < -1 || src[b][k] >= c->n) return fail(RM_ERR_INVALID, "source index out of range (-1 .. n_nodes-1)");
        total += size_t(n_src[b]);
    }
    RM_HIP(hipSetDevice(c->device));
    double *h_energy = nullptr;
    int32_t *h_src = nullptr;
    uint8_t *h_flags = nullptr;
    static thread_local std::vector<const int32_t *> lists;
    lists.assign(size_t(n_ticks), nullptr);
    if (total > 0) {
        RM_TRY(energy_host_block(c, int32_t(total), &h_energy, &h_src, &h_flags));
        size_t at = 0;
        for (int b = 0; b < n_ticks; ++b) {
            if (n_src[b] > 0) std::memcpy(h_src + at, src[b], size_t(n_src[b]) * 4);
            lists[size_t(b)] = h_src + at;
            at += size_t(n_src[b]);
        }
    }
    RM_TRY(cca_batch(c, n_ticks, t_begin_us, t_end_us, lists.data(), n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, h_flags, h_energy));
    RM_HIP(hipStreamSynchronize(c->stream));
    if (total > 0 && cca_flags) std::memcpy(cca_flags, h_flags, total);
    if (total > 0 && cca_energy_dbm) std::memcpy(cca_energy_dbm, h_energy, total * 8);
    return RM_OK;
}

int rm_tick_run_sources_cca_device(rm_context *c, int64_t t_begin_us, int64_t t_end_us, const int32_t *dev_src, int32_t n, int64_t start_us,
                                   int64_t air_us, int64_t cca_time_us, double cca_threshold_dbm, uint8_t *dev_cca_flags,
                                   double *dev_cca_energy_dbm)
{
    RM_TRY(cca_check(c, t_begin_us, dev_src, n, start_us, air_us, cca_time_us));
    return cca_tick(c, t_begin_us, t_end_us, dev_src, n, start_us, air_us, cca_time_us, cca_threshold_dbm, dev_cca_flags, dev_cca_energy_dbm);
}

int rm_tick_run_sources_cca(rm_context *c, int64_t t_begin_us, int64_t t_end_us, const int32_t *src, int32_t n, int64_t start_us,
                            int64_t air_us, int64_t cca_time_us, double cca_threshold_dbm, uint8_t *cca_flags, double *cca_energy_dbm)
{
    RM_TRY(cca_check(c, t_begin_us, src, n, start_us, air_us, cca_time_us));
    for (int32_t k = 0; k < n; ++k)
        if (src[k] < -1 || src[k] >= c->n) return fail(RM_ERR_INVALID, "source index out of range (-1 .. n_nodes-1)");
    RM_HIP(hipSetDevice(c->device));
    double *h_energy = nullptr;
    int32_t *h_src = nullptr;
    uint8_t *h_flags = nullptr;
    if (n > 0) {
        RM_TRY(energy_host_block(c, n, &h_energy, &h_src, &h_flags));
        std::memcpy(h_src, src, size_t(n) * 4);
    }
    RM_TRY(cca_tick(c, t_begin_us, t_end_us, h_src, n, start_us, air_us, cca_time_us, cca_threshold_dbm, h_flags, h_energy));
    RM_HIP(hipStreamSynchronize(c->stream));
    if (n > 0 && cca_flags) std::memcpy(cca_flags, h_flags, size_t(n));
    if (n > 0 && cca_energy_dbm) std::memcpy(cca_energy_dbm, h_energy, size_t(n) * 8);
    return RM_OK;
}

} // extern "C"
