// rm_api_cca.cpp -- C ABI: the carrier-sense gated tick (rm_tick_run_sources_cca*; k_cca_gate in rm_energy.hip).
//
// One call: the candidates are sensed on the device over the on-air window as it is when the tick begins (E5 at cca_time_us, each on
// its own channel), the ones that find the channel busy -- or are on the air themselves -- become padding entries of a source list
// the context owns, and the unchanged SINR lone tick runs over that list.  Everything is ordered on the context's stream; the host
// learns nothing in between.
#include "rm_host.hpp"

using namespace rmh;

namespace {

// what both forms refuse, before anything is launched and with nothing changed
int cca_check(rm_context *c, int64_t t_begin_us, const int32_t *src, int32_t n, int64_t start_us, int64_t air_us, int64_t cca_time_us)
{
    if (!c || n < 0 || (n > 0 && !src) || air_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(energy_check(c, cca_time_us, n, true));
    if (cca_time_us < t_begin_us)
        return fail(RM_ERR_INVALID, "cca_time_us is earlier than t_begin_us: frames that had left the air by then are gone");
    if (cca_time_us > start_us)
        return fail(RM_ERR_INVALID, "cca_time_us is later than start_us: the sample would have to see the frames of this very call");
    if (air_us > int64_t(UINT32_MAX)) return fail(RM_ERR_INVALID, "a frame of the SINR medium has to be shorter than 2^32 us");
    return RM_OK;
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

} // namespace

extern "C" {

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
