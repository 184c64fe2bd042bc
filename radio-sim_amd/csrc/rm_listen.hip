// rm_listen.hip -- receiver listening schedules: a pass over the FINISHED result
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// A duty-cycled receiver that sleeps at a frame's first microsecond does not get the frame.  Every decision site is left as it is:
// a link's verdict is final under everything else (Tx failure, capture, half duplex, the draws, the frame error model's pass) when
// this pass runs, and the pass turns RM_DELIVERED into RM_INTERFERED where the receiver's schedule says it slept at the frame's
// start, adding 1 to the receiver's missed count.  One lane per heard link of a result slot's compact arrays; a batch is one launch
// over all of its slots (blockIdx.y).  The pass reads the verdict byte first: a link that is not RM_DELIVERED leaves before any
// 64-bit work, and one whose receiver always listens leaves after one load.  It writes nothing but verdict bytes and the counts.
#include "rm_device.hpp"

namespace rm {

bool host_listen_valid(const rm_listen_schedule &s) { return listen_valid(s); }
bool host_listen_at(const rm_listen_schedule &s, int64_t t_us) { return listen_at(s, t_us); }

// Workgroups per slot, as the frame error model's pass: 16 384 lanes per stride over the slot's links (not tuned).
constexpr int kListenBlocks = 64;

RM_D void listen_body(const ListenDev &ld, const TickDev &t)
{
    // a slot that overflowed its capacity or was dropped is left as it is and counts nothing; an empty tick has no links
    if (!t.out_count || !t.out_verdict || !t.out_pkt || !t.out_dst || !t.tx) return;
    if (t.out_count[1] != 0u || (t.stage_count && t.stage_count[1] != 0u)) return;
    const uint32_t n = min(t.out_count[0], t.out_count[2]);
    const int n_new = t.n_active - t.first_new;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (t.out_verdict[i] != uint8_t(RM_DELIVERED)) continue;
        const int32_t dst = t.out_dst[i];
        if (dst < 0 || dst >= ld.n_nodes) continue; // (results may come from the caller's records: never outside the tables)
        const rm_listen_schedule *sp = ld.sched + dst;
        const int64_t period = sp->period_us;
        if (period == 0) continue; // always listening: one load
        const int q = t.out_pkt[i];
        if (q < 0 || q >= n_new) continue;
        rm_listen_schedule sc;
        sc.period_us = period;
        sc.on_us = sp->on_us;
        sc.phase_us = sp->phase_us;
        if (listen_at(sc, t.tx[t.first_new + q].start_us)) continue;
        t.out_verdict[i] = uint8_t(RM_INTERFERED);
        (void)atomicAdd(reinterpret_cast<unsigned long long *>(ld.missed + dst), 1ull);
    }
}

__global__ void __launch_bounds__(256) k_listen(const ListenDev ld, const TickDev t) { listen_body(ld, t); }
__global__ void __launch_bounds__(256) k_listen_batch(const ListenDev ld, const TickDev *__restrict__ ticks) { listen_body(ld, ticks[blockIdx.y]); }

hipError_t launch_listen(hipStream_t s, const ListenDev &ld, const TickDev &t)
{
    RM_KLAUNCH(k_listen, dim3(kListenBlocks), dim3(256), 0, s, ld, t);
    return hipGetLastError();
}

hipError_t launch_listen_batch(hipStream_t s, const ListenDev &ld, int n, const TickDev *dev_ticks)
{
    if (n < 1 || n > kMaxBatch) return hipErrorInvalidValue;
    RM_KLAUNCH(k_listen_batch, dim3(kListenBlocks, n), dim3(256), 0, s, ld, dev_ticks);
    return hipGetLastError();
}

} // namespace rm
