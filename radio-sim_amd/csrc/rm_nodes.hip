// rm_nodes.hip -- the node table on the device: receiver pre-filter records and boxes, changed nodes in place, Tx packing
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
#include "rm_device.hpp"

namespace rm {

// Pre-filter record per receiver: (fx, fy, fz, channel bits) in the fp32 frame; a disabled radio
// gets a NaN position so that the geometric test can never pass (Transciever.isEnabled(),
// UDGMRadioMedium.java:102).  One wave per group of 64 receivers; the group's bounding box is the
// min/max of exactly these fp32 coordinates, so the box test is conservative w.r.t. the
// per-receiver test by monotonicity of fp32 rounding.
__global__ void __launch_bounds__(64) k_prep_rx(NodesDev nd, ModelDev m)
{
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int i = g * kGroup + lane;
    const bool geometric = (m.kind == RM_MODEL_UDGM || m.kind == RM_MODEL_UDGM_CONST || m.kind == RM_MODEL_LOGDIST);
    const float nanf_ = __builtin_nanf("");
    const float inf_ = __builtin_inff();
    float4 r;
    r.x = r.y = r.z = nanf_;
    r.w = 0.f;
    if (i < nd.n_rx) {
        if (nd.enabled[i]) {
            if (geometric) {
                r.x = float(nd.x[i] - m.org_x);
                r.y = float(nd.y[i] - m.org_y);
                r.z = float(nd.z[i] - m.org_z);
            } else {
                r.x = r.y = r.z = 0.f;
            }
        }
        r.w = __int_as_float(nd.channel[i]);
        nd.rxf[i] = r;
    }
    const bool ok = (r.x == r.x);
    const float lox = wave_min(ok ? r.x : inf_), hix = wave_max(ok ? r.x : -inf_);
    const float loy = wave_min(ok ? r.y : inf_), hiy = wave_max(ok ? r.y : -inf_);
    const float loz = wave_min(ok ? r.z : inf_), hiz = wave_max(ok ? r.z : -inf_);
    // the channels heard in the group: bit (channel & 31) of every receiver that can be a candidate at all
    uint32_t chm = (ok && i < nd.n_rx) ? (1u << (uint32_t(nd.channel[min(i, nd.n_rx - 1)]) & 31u)) : 0u;
    for (int d = 32; d >= 1; d >>= 1) chm |= uint32_t(__shfl_xor(int(chm), d));
    if (lane == 0) {
        nd.bbox_xy[g] = make_float4(lox, loy, hix, hiy);
        nd.bbox_z[g] = make_float2(loz, hiz);
        nd.grp_chmask[g] = chm;
    }
}

// union of the 16 group boxes of one filter workgroup (4 waves x 4 groups = 1024 receivers)
__global__ void __launch_bounds__(256) k_wg_boxes(NodesDev nd, int n_wg)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_wg) return;
    const int n_groups = (nd.n_rx + kGroup - 1) / kGroup;
    BoxUnion u = box_union_empty();
    for (int g = b * 16; g < min(n_groups, b * 16 + 16); ++g) box_union_add(u, nd.bbox_xy[g], nd.bbox_z[g], nd.grp_chmask[g]);
    nd.wg_box_xy[b] = u.xy;
    nd.wg_box_z[b] = u.z;
    nd.wg_chmask[b] = u.chmask;
}

// Changed nodes written in place: the source table by node index, the receiver table (SoA arrays
// and the exact-path record) at the node's engine position.  The engine order stays as it is --
// it only has to be a permutation; k_prep_rx recomputes the pre-filter records and boxes afterwards.
__global__ void __launch_bounds__(256) k_patch_nodes(NodesDev nd, const NodePatch *list, int n, NodePatch one)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const NodePatch p = list ? list[i] : one;
    const_cast<double *>(nd.sx)[p.node] = p.x;
    const_cast<double *>(nd.sy)[p.node] = p.y;
    const_cast<double *>(nd.sz)[p.node] = p.z;
    const_cast<double *>(nd.stxpower)[p.node] = p.txpower;
    const_cast<double *>(nd.stxprob)[p.node] = p.txprob;
    const_cast<double *>(nd.srxprob)[p.node] = p.rxprob;
    const_cast<int32_t *>(nd.schannel)[p.node] = p.channel;
    const_cast<uint8_t *>(nd.senabled)[p.node] = uint8_t(p.enabled);
    SrcRecord *sr = const_cast<SrcRecord *>(nd.srec) + p.node;
    sr->x = p.x;
    sr->y = p.y;
    sr->z = p.z;
    sr->txpower = p.txpower;
    sr->txprob = p.txprob;
    sr->channel = p.channel;
    if (p.pos < 0) return;
    const_cast<double *>(nd.x)[p.pos] = p.x;
    const_cast<double *>(nd.y)[p.pos] = p.y;
    const_cast<double *>(nd.z)[p.pos] = p.z;
    const_cast<double *>(nd.rxprob)[p.pos] = p.rxprob;
    const_cast<int32_t *>(nd.channel)[p.pos] = p.channel;
    const_cast<uint8_t *>(nd.enabled)[p.pos] = uint8_t(p.enabled);
    RxRecord *r = const_cast<RxRecord *>(nd.rec) + p.pos;
    r->x = p.x;
    r->y = p.y;
    r->z = p.z;
    r->rxprob = p.rxprob;
    r->channel = p.channel;
    r->enabled = p.enabled;
    if (!nd.rec32) return;
    RxCompact *c = const_cast<RxCompact *>(nd.rec32) + p.pos;
    c->x = p.x;
    c->y = p.y;
    c->z = p.z;
    c->flags = (p.rxprob != 1.0) ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
k_pack_tx(NodesDev nd, const int32_t *src, int n, int64_t start_us, int64_t air_us, rm_tx_record *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rm_tx_record r = make_tx_record(nd, src[i], start_us, air_us);
    out[i] = r;
}

constexpr int kPackChunk = 128; // ticks per k_pack_tx_batch launch: their start times travel in the kernel arguments (1 KB)
struct PackStarts {
    int64_t start_us[kPackChunk];
};

// (blockIdx.z: the rank whose [n_ticks][n] block of source indices this is -- one block when a rank packs its own
// transmitters, `world` of them when the INDICES were all-gathered and every rank builds all records itself: 4 bytes per
// frame over the links between the GPUs instead of 64)
__global__ void __launch_bounds__(256)
k_pack_tx_batch(NodesDev nd, const int32_t *src, int n, PackStarts st, int64_t air_us, rm_tx_record *out, int tick0, int n_ticks)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t(blockIdx.z) * n_ticks + size_t(tick0 + blockIdx.y)) * n + i;
    const rm_tx_record r = make_tx_record(nd, src[o], st.start_us[blockIdx.y], air_us);
    out[o] = r;
}

// a rank's block of a sharded batch as it goes into the all-gather: its source indices, then the trailer (the node table's
// digest in two words, two spare words)
__global__ void __launch_bounds__(256) k_stage_block(const int32_t *__restrict__ src, int n, uint64_t digest, int32_t *__restrict__ dst)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
    if (i == 0) {
        dst[n] = int32_t(uint32_t(digest));
        dst[n + 1] = int32_t(uint32_t(digest >> 32));
        dst[n + 2] = 0;
        dst[n + 3] = 0;
    }
}

hipError_t launch_stage_block(hipStream_t s, const int32_t *src, int n, uint64_t digest, int32_t *dst)
{
    RM_KLAUNCH(k_stage_block, dim3(cdiv(max(n, 1), 256)), dim3(256), 0, s, src, n, digest, dst);
    return hipGetLastError();
}

hipError_t launch_patch_nodes(hipStream_t s, const NodesDev &nd, const NodePatch *dev_list, int n, const NodePatch &one)
{
    if (n <= 0) return hipSuccess;
    RM_KLAUNCH(k_patch_nodes, dim3(cdiv(n, 256)), dim3(256), 0, s, nd, dev_list, n, one);
    return hipGetLastError();
}

hipError_t launch_prep_rx(hipStream_t s, const NodesDev &nd, const ModelDev &m)
{
    if (nd.n_rx <= 0) return hipSuccess;
    RM_KLAUNCH(k_prep_rx, dim3(cdiv(nd.n_rx, kGroup)), dim3(64), 0, s, nd, m);
    const int n_wg = cdiv(nd.n_rx, kGroup * 16);
    RM_KLAUNCH(k_wg_boxes, dim3(cdiv(n_wg, 256)), dim3(256), 0, s, nd, n_wg);
    return hipGetLastError();
}

hipError_t launch_pack_tx(hipStream_t s, const NodesDev &nd, const int32_t *dev_src, int n, int64_t start_us,
                          int64_t air_us, rm_tx_record *out)
{
    if (n <= 0) return hipSuccess;
    RM_KLAUNCH(k_pack_tx, dim3(cdiv(n, 256)), dim3(256), 0, s, nd, dev_src, n, start_us, air_us, out);
    return hipGetLastError();
}

hipError_t launch_pack_tx_batch(hipStream_t s, const NodesDev &nd, const int32_t *dev_src, int n_ticks, int n,
                                const int64_t *start_us, int64_t air_us, rm_tx_record *out, int world)
{
    if (n <= 0 || n_ticks <= 0) return hipSuccess;
    if (n_ticks > kMaxBatch) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < n_ticks; b0 += kPackChunk) {
        const int nb = min(kPackChunk, n_ticks - b0);
        PackStarts st{};
        for (int b = 0; b < nb; ++b) st.start_us[b] = start_us[b0 + b];
        RM_KLAUNCH(k_pack_tx_batch, dim3(cdiv(n, 256), nb, max(world, 1)), dim3(256), 0, s, nd, dev_src, n, st, air_us, out, b0, n_ticks);
    }
    return hipGetLastError();
}

} // namespace rm
