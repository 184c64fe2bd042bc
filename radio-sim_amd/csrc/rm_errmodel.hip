// rm_errmodel.hip -- the frame error model of the SINR medium: a pass over the FINISHED result
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The decision sites of the SINR medium (air_sinr, sinr_body / k_sinr_acc_batch, the tick by scan, k_ov_verdict) are left as they
// are: a link's verdict is final under everything they know when this pass runs, and the pass turns RM_DELIVERED into
// RM_INTERFERED where the link's draw does not fall below the frame's packet success ratio.  One lane per heard link of a result
// slot's compact arrays; a batch is one launch over all of its slots (blockIdx.y).  The pass reads the verdict byte first: a link
// that is not RM_DELIVERED leaves before any 64-bit work.  It writes nothing but verdict bytes.
#include "rm_device.hpp"

namespace rm {

double host_em_psr(int kind, double us_per_bit, double sinr_db, int64_t air_us)
{
    return kind == RM_EM_OQPSK_250K ? em_psr_oqpsk(us_per_bit, sinr_db, air_us) : 1.0;
}
double host_em_draw(uint64_t seed, int32_t src, int64_t start_us, int32_t dst) { return em_draw(seed, src, start_us, dst); }

// Workgroups per slot: 16 384 lanes per stride over the slot's links.  A batch multiplies it by its slots; a lone tick of very many links
// (the capacity allows 4 M) walks them in strides on a quarter of the CUs, and lanes whose links are not RM_DELIVERED idle while
// their wave's survivors run the fp64 chain (no compaction).  Both are OPEN MEASUREMENTS, not tuned choices.
constexpr int kEmBlocks = 64;

RM_D void errmodel_body(const EmDev &em, const TickDev &t)
{
    // a slot that overflowed its capacity or was dropped is left as it is; an empty tick has no links
    if (!t.out_count || !t.out_verdict || !t.out_sinr || !t.out_pkt) return;
    if (t.out_count[1] != 0u || (t.stage_count && t.stage_count[1] != 0u)) return;
    const uint32_t n = min(t.out_count[0], t.out_count[2]);
    const int n_new = t.n_active - t.first_new;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (t.out_verdict[i] != uint8_t(RM_DELIVERED)) continue;
        const int q = t.out_pkt[i];
        if (q < 0 || q >= n_new) continue;
        const rm_tx_record *rec = t.tx + t.first_new + q;
        const int32_t src = rec->src;
        if (src < 0) continue; // (a padding record has an empty segment)
        const double sinr_db = t.out_sinr[i];
        // The shortcut the spec allows: every exponent of the sum is at most that of k = 2 (1/k - 1 is most negative at k = 16 and the
        // roundings are monotone), and det_exp2 returns 0 below -1022 -- then acc = 0, ber = 0, 1 - ber = 1, psr = det_exp2(n * 0) = 1
        // and u < 1 always: the link stays delivered.  (A NaN fails the comparison and takes the formula.)
        const double s = det_pow10(sinr_db / 10.0);
        const double y2 = ((20.0 * s) * (1.0 / 2.0 - 1.0)) * 1.4426950408889634;
        if (y2 < -1022.0) continue;
        const double ber = em_ber_oqpsk(s);
        double psr = ber;
        if (ber == ber) psr = det_exp2((double(rec->air_us) / em.us_per_bit) * det_log2(1.0 - ber));
        const double u = em_draw(em.seed, src, rec->start_us, t.out_dst[i]);
        if (!(u < psr)) t.out_verdict[i] = uint8_t(RM_INTERFERED);
    }
}

__global__ void __launch_bounds__(256) k_errmodel(const EmDev em, const TickDev t) { errmodel_body(em, t); }
__global__ void __launch_bounds__(256) k_errmodel_batch(const EmDev em, const TickDev *__restrict__ ticks) { errmodel_body(em, ticks[blockIdx.y]); }

hipError_t launch_errmodel(hipStream_t s, const EmDev &em, const TickDev &t)
{
    RM_KLAUNCH(k_errmodel, dim3(kEmBlocks), dim3(256), 0, s, em, t);
    return hipGetLastError();
}

hipError_t launch_errmodel_batch(hipStream_t s, const EmDev &em, int n, const TickDev *dev_ticks)
{
    RM_KLAUNCH(k_errmodel_batch, dim3(kEmBlocks, n), dim3(256), 0, s, em, dev_ticks);
    return hipGetLastError();
}

} // namespace rm
