// rm_api_energy.cpp -- C ABI: the channel energy query (rm_channel_energy*; kernels in rm_energy.hip).
//
// The query READS the SINR medium's on-air window (d_air[air_head, air_tail)) and the node table and writes the caller's
// outputs and scratch of its own (rm_context::Energy): no tick slot, no result buffer, no on-air list, not ev.gen, not the
// generator, not air_max_t_begin.  A tick, a batch or a drain after a query gives what it gave without one.
#include "rm_host.hpp"

using namespace rmh;

namespace rmh {

// what both forms refuse, before anything is launched
int energy_check(rm_context *c, int64_t time_us, int32_t n, bool have_list)
{
    if (!c) return fail(RM_ERR_INVALID, "ctx is NULL");
    if (n < 0) return fail(RM_ERR_INVALID, "negative node count");
    if (!is_sinr(c))
        return fail(RM_ERR_STATE, "channel energy is a query over the frames on the air: only the log-distance medium with RM_LD_SINR keeps them");
    if (c->in_tick) return fail(RM_ERR_STATE, "rm_channel_energy between rm_tick_begin and rm_tick_flush");
    if (part_count(c) != c->n || part_spatial(c))
        return fail(RM_ERR_STATE, "channel energy needs the whole receiver table: this context has a receiver partition");
    if (c->air_culled)
        return fail(RM_ERR_STATE, "the frames on the air were selected for a region (a gathered batch): the window does not hold them all");
    if (time_us < c->air_max_t_begin)
        return fail(RM_ERR_INVALID, "time_us is earlier than the latest tick over the on-air window: frames that had left the air by then are gone");
    if (!have_list && n > c->n) return fail(RM_ERR_INVALID, "more nodes than the table holds");
    return RM_OK;
}

// index + sum (or, with `gated`, index + gate) on the context's stream; nodes / energy / flags are device-visible memory
int energy_launch(rm_context *c, int64_t time_us, const int32_t *nodes, int32_t n, int32_t channel, double cca_threshold, double *energy,
                  uint8_t *flags, int32_t *gated)
{
    RM_TRY(prepare_nodes(c)); // pending node changes first, as a tick does
    if (c->n_rx != c->n) return fail(RM_ERR_STATE, "internal: the receiver table does not hold every node");
    rm_context::Energy &e = c->ed;
    const size_t n_win = c->air_tail - c->air_head;
    if (n_win > size_t(INT32_MAX)) return fail(RM_ERR_CAPACITY, "on-air window too large");
    const bool grid = n_win >= size_t(rm::kEdSmallWindow);
    const size_t cnt_len = 2 + size_t(rm::kEdCells);
    RM_HIP(e.cnt.ensure(cnt_len));
    RM_HIP(e.every_f.ensure(std::max<size_t>(n_win, 1)));
    RM_HIP(e.every_m.ensure(std::max<size_t>(n_win, 1)));
    if (grid) {
        RM_HIP(e.bucket_f.ensure(size_t(rm::kEdCells) * rm::kEdK));
        RM_HIP(e.bucket_m.ensure(size_t(rm::kEdCells) * rm::kEdK));
    }
    if (e.tx_mark.n < size_t(std::max(c->n, 1))) { // (a fresh array knows no stamp)
        RM_HIP(e.tx_mark.ensure(size_t(std::max(c->n, 1))));
        RM_HIP(hipMemsetAsync(e.tx_mark.p, 0, e.tx_mark.n * sizeof(uint32_t), c->stream));
    }
    if (++e.stamp == 0u) { // (the stamps have gone round: forget the old ones)
        e.stamp = 1u;
        RM_HIP(hipMemsetAsync(e.tx_mark.p, 0, e.tx_mark.n * sizeof(uint32_t), c->stream));
    }
    // the index is built from scratch: the list's count and the largest radius always, the cells' counts when there is a grid
    RM_HIP(hipMemsetAsync(e.cnt.p, 0, (grid ? cnt_len : 2) * sizeof(uint32_t), c->stream));
    rm::EnergyDev ed{};
    ed.cnt = e.cnt.p;
    ed.bucket_f = e.bucket_f.p;
    ed.bucket_m = e.bucket_m.p;
    ed.every_f = e.every_f.p;
    ed.every_m = e.every_m.p;
    ed.tx_mark = e.tx_mark.p;
    ed.stamp = e.stamp;
    ed.half = std::max(float(c->coord_bound), 1e-20f);
    ed.inv = float(rm::kEdG) / (2.0f * ed.half);
    rm::ModelDev m = model_dev(c);
    if (c->f32_slack > 0.05) m.shadow_tbl = nullptr; // (as the sweep: the link-hash table goes with the fp32 filter of a small frame)
    CallProbe probe(c); // (rm_profile_kernels names the path that ran)
    sample_stage(probe.smp, RM_STAGE_SINR);
    if (gated)
        RM_HIP(rm::launch_cca_gate(c->stream, nodes_dev(c), m, c->d_air.p + c->air_head, int(n_win), time_us, ed, grid, nodes, n, cca_threshold,
                                   gated, energy, flags));
    else
        RM_HIP(rm::launch_energy(c->stream, nodes_dev(c), m, c->d_air.p + c->air_head, int(n_win), time_us, ed, grid, nodes, n, channel,
                                 cca_threshold, energy, flags));
    return RM_OK;
}

// one pinned, host-mapped block: the list in, energies and flags out -- the kernels read and write it in place (a lock-stepped
// host asks for a few hundred nodes per tick: one small launch sequence and one synchronisation, no copy engine in between)
int energy_host_block(rm_context *c, int32_t n, double **h_energy, int32_t **h_nodes, uint8_t **h_flags)
{
    rm_context::Energy &e = c->ed;
    if (e.h_cap < size_t(n)) {
        RM_HIP(hipStreamSynchronize(c->stream));
        if (e.h_block) RM_HIP(hipHostFree(e.h_block));
        e.h_block = nullptr;
        e.h_cap = 0;
        const size_t want = std::max<size_t>(size_t(n) + size_t(n) / 2, 1024);
        RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&e.h_block), pad64(want * 8) + pad64(want * 4) + pad64(want), hipHostMallocMapped));
        e.h_cap = want;
    }
    *h_energy = reinterpret_cast<double *>(e.h_block);
    *h_nodes = reinterpret_cast<int32_t *>(e.h_block + pad64(e.h_cap * 8));
    *h_flags = reinterpret_cast<uint8_t *>(e.h_block + pad64(e.h_cap * 8) + pad64(e.h_cap * 4));
    return RM_OK;
}

} // namespace rmh

extern "C" {

int rm_channel_energy_device(rm_context *c, int64_t time_us, const int32_t *dev_nodes, int32_t n, int32_t channel, double cca_threshold_dbm,
                             double *dev_energy_dbm, uint8_t *dev_flags)
{
    RM_TRY(energy_check(c, time_us, n, dev_nodes != nullptr));
    if (n == 0) return RM_OK;
    if (!dev_energy_dbm) return fail(RM_ERR_INVALID, "dev_energy_dbm is NULL");
    RM_HIP(hipSetDevice(c->device));
    return energy_launch(c, time_us, dev_nodes, n, channel, cca_threshold_dbm, dev_energy_dbm, dev_flags);
}

int rm_channel_energy(rm_context *c, int64_t time_us, const int32_t *nodes, int32_t n, int32_t channel, double cca_threshold_dbm,
                      double *energy_dbm, uint8_t *flags)
{
    RM_TRY(energy_check(c, time_us, n, nodes != nullptr));
    if (n == 0) return RM_OK;
    if (!energy_dbm) return fail(RM_ERR_INVALID, "energy_dbm is NULL");
    if (nodes)
        for (int32_t k = 0; k < n; ++k)
            if (nodes[k] < 0 || nodes[k] >= c->n) return fail(RM_ERR_INVALID, "node index out of range");
    RM_HIP(hipSetDevice(c->device));
    double *h_energy;
    int32_t *h_nodes;
    uint8_t *h_flags;
    RM_TRY(energy_host_block(c, n, &h_energy, &h_nodes, &h_flags));
    if (nodes) std::memcpy(h_nodes, nodes, size_t(n) * 4);
    RM_TRY(energy_launch(c, time_us, nodes ? h_nodes : nullptr, n, channel, cca_threshold_dbm, h_energy, h_flags));
    RM_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(energy_dbm, h_energy, size_t(n) * 8);
    if (flags) std::memcpy(flags, h_flags, size_t(n));
    return RM_OK;
}

} // extern "C"
