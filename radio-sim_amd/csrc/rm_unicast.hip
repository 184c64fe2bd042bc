// rm_unicast.hip -- the unicast outcome query: a read-only pass over FINISHED results
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// One launch per query, a lane per entry, grid-stride.  An entry names a result slot, a packet of it and a wanted node; the lane
// binary-searches the packet's segment of dst (ascending: the result's promise) for the node and writes the five outputs with plain
// stores.  Neighbouring lanes hold neighbouring packets and so neighbouring segments: the first probes of a wave fall into few
// lines, the last ones into the lanes' own.  No atomics, no cross-lane traffic, nothing written outside the caller's arrays.
// The slots form finds a lane's slot by an upper bound over the prefix of the entries per slot, staged in LDS once per workgroup
// (at most RM_MAX_BATCH + 1 words; the lanes of a wave probe the same few words: broadcasts, not conflicts).
// Untuned: the link-parallel shape -- a lane per heard link -- has not been measured against this one.
#include "rm_device.hpp"

namespace rm {

constexpr int kUcThreads = 256;
constexpr int kUcMaxBlocks = 2048;

RM_D double uc_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// entry e: packet p of the slot described by s (have: there is such a slot), wanted node w
RM_D void uc_entry(const UcSlot &s, bool have, int p, int w, int n_nodes, uint64_t e, const rm_unicast_out &o)
{
    int32_t link = -1, reply = -1;
    double rssi = uc_nan(), sinr = uc_nan();
    const int status = have ? uc_find(s, p, w, n_nodes, link) : int(RM_UC_NONE); // (the search: rm_device.hpp)
    if (link >= 0) {
        if (status == RM_UC_DELIVERED) reply = w;
        if (s.rssi) rssi = s.rssi[link];
        if (s.sinr) sinr = s.sinr[link];
    }
    if (o.status) o.status[e] = uint8_t(status);
    if (o.link) o.link[e] = link;
    if (o.rssi) o.rssi[e] = rssi;
    if (o.sinr) o.sinr[e] = sinr;
    if (o.reply_src) o.reply_src[e] = reply;
}

__global__ void __launch_bounds__(kUcThreads) k_unicast_slots(const UcSlot *__restrict__ slots, const UcSlot lone, int n_slots,
                                                              const uint32_t *__restrict__ prefix, uint64_t n, int n_nodes,
                                                              const int32_t *__restrict__ want, const rm_unicast_out o)
{
    __shared__ uint32_t pre[kMaxBatch + 1];
    if (prefix) {
        for (int k = int(threadIdx.x); k <= n_slots; k += kUcThreads) pre[k] = prefix[k];
        __syncthreads();
    }
    const uint64_t stride = uint64_t(gridDim.x) * kUcThreads;
    for (uint64_t e = uint64_t(blockIdx.x) * kUcThreads + threadIdx.x; e < n; e += stride) {
        int b = 0;
        uint32_t p = uint32_t(e);
        if (prefix) { // the slot of entry e: the last b with pre[b] <= e (slots without entries are stepped over)
            int lo = 1, hi = n_slots; // first j in [1, n_slots] with pre[j] > e; pre[n_slots] == n > e
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (pre[mid] > uint32_t(e)) hi = mid;
                else lo = mid + 1;
            }
            b = lo - 1;
            p = uint32_t(e) - pre[b];
        }
        const UcSlot s = slots ? slots[b] : lone; // (a wave's lanes mostly share the slot: the same few lines)
        uc_entry(s, true, int(p), want[e], n_nodes, e, o);
    }
}

__global__ void __launch_bounds__(kUcThreads) k_unicast_at(const UcSlot *__restrict__ slots, const UcSlot lone, int n_slots, uint64_t n, int n_nodes,
                                                           const int32_t *__restrict__ slot, const int32_t *__restrict__ pkt,
                                                           const int32_t *__restrict__ want, const rm_unicast_out o)
{
    const uint64_t stride = uint64_t(gridDim.x) * kUcThreads;
    for (uint64_t e = uint64_t(blockIdx.x) * kUcThreads + threadIdx.x; e < n; e += stride) {
        const int b = slot[e];
        const bool have = b >= 0 && b < n_slots;
        const UcSlot s = (have && slots) ? slots[b] : lone;
        uc_entry(s, have, pkt[e], want[e], n_nodes, e, o);
    }
}

static int uc_blocks(int64_t n) { return int(std::max<int64_t>(1, std::min<int64_t>(kUcMaxBlocks, (n + kUcThreads - 1) / kUcThreads))); }

hipError_t launch_unicast_slots(hipStream_t s, const UcSlot *dev_slots, const UcSlot &lone, int n_slots, const uint32_t *dev_prefix, int64_t n,
                                int n_nodes, const int32_t *want, const rm_unicast_out &out)
{
    if (n <= 0) return hipSuccess;
    if (n_slots < 1 || n_slots > kMaxBatch || n > (int64_t(1) << 27) || !want || (n_slots > 1 && (!dev_slots || !dev_prefix))) return hipErrorInvalidValue;
    RM_KLAUNCH(k_unicast_slots, dim3(uc_blocks(n)), dim3(kUcThreads), 0, s, dev_slots, lone, n_slots, dev_prefix, uint64_t(n), n_nodes, want, out);
    return hipGetLastError();
}

hipError_t launch_unicast_at(hipStream_t s, const UcSlot *dev_slots, const UcSlot &lone, int n_slots, int64_t n, int n_nodes,
                             const int32_t *slot, const int32_t *pkt, const int32_t *want, const rm_unicast_out &out)
{
    if (n <= 0) return hipSuccess;
    if (n_slots < 1 || n_slots > kMaxBatch || n > (int64_t(1) << 27) || !slot || !pkt || !want || (n_slots > 1 && !dev_slots)) return hipErrorInvalidValue;
    RM_KLAUNCH(k_unicast_at, dim3(uc_blocks(n)), dim3(kUcThreads), 0, s, dev_slots, lone, n_slots, uint64_t(n), n_nodes, slot, pkt, want, out);
    return hipGetLastError();
}

} // namespace rm
