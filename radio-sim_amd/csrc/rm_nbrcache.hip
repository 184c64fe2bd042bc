// rm_nbrcache.hip -- the source cache of the batched sweep (NbrCacheDev): claim, fill, publish, expand
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
#include "rm_device.hpp"

namespace rm {

// ============================================================================ the source cache (NbrCacheDev)
// Three kernels, in both forms of the cache: claim (a swept frame's source gets a list), fill (the list's entries), expand (a
// frame the pre-pass took out of the sweep gets what its source's list holds).  A candidates list written here is read by LATER
// launch sequences of the same context only (the pre-pass of this one has run), so the order of the stream is all the ordering
// there is.  A heard list lies in a pool that several contexts, each on its stream, read and fill: a fourth kernel, publish,
// makes it valid behind the fill (rm_engine.h: NbrCacheDev).
// Heard form (t.nc.arena_rssi != nullptr, block-uniform in every kernel below): expand alone runs before the exact stage and
// only hands the hit frames' list lengths to the reorder stage's scan; claim and fill run BEHIND the reorder stage (and
// k_reorder_served_batch, rm_reorder.hip) and take the swept frames' finished records from the ordered arrays.
// Candidates form: all three run between the sweep and the exact stage, over the candidates the sweep has appended.

// one thread per frame: a swept frame whose source has no list in this epoch claims one (compare-and-swap on the state word: a
// node that transmits in two ticks of the batch is filled once) and takes its room from the arena.  A source with more
// candidates than kNcListCap, or one the arena has no room for, keeps the claim and stays uncached for the epoch.
// Heard form, a tick with hits: one thread per entry of the tick's list of unserved frames instead (nc.unserved, rm_engine.h).
__global__ void __launch_bounds__(256) k_nc_claim_batch(const TickDev *__restrict__ ticks)
{
    const TickDev &t = ticks[blockIdx.z];
    if (t.nc.state == nullptr) return;
    const int n_eval = t.n_active - t.first_eval;
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) {
        atomicAdd(&t.nc.ctr[1], (unsigned long long)t.nc.tick_cnt[2]);
        atomicAdd(&t.nc.ctr[2], (unsigned long long)t.nc.tick_cnt[0]);
    }
    const bool heard = t.nc.arena_rssi != nullptr;
    // heard form: every frame of the tick was served -- each has a hit, none can claim (block-uniform).  Nothing is written:
    // tick_cnt[1] stays 0, so k_nc_fill_batch returns before it reads fill[], which is NOT cleared between launch sequences --
    // a tick that goes on below therefore writes fill[e] for every one of its frames.
    if (heard && uniform_u(t.nc.tick_cnt[2]) == uint32_t(n_eval)) return;
    // heard form, a tick with hits: thread k takes the k-th entry of the tick's list of frames without a hit (nc.unserved; the
    // pre-pass left n_un = tick_cnt[3] of them) and fill[] goes by that position -- the fill reads it the same way, and every
    // position below n_un is written, so the rule above holds for the list as it held for the frames.  A tick without a hit has
    // no list to follow: position k is frame k.  Workgroups beyond the list have nothing to look at (block-uniform).
    const bool listed = heard && uniform_u(t.nc.tick_cnt[2]) != 0u;
    const int n_walk = listed ? min(int(uniform_u(t.nc.tick_cnt[3])), n_eval) : n_eval;
    if (int(blockIdx.x * blockDim.x) >= n_walk) return;
    const int k = e; // the thread's position: in the list, or among the frames
    if (listed) e = k < n_walk ? t.nc.unserved[k] : n_eval;
    const int lane = threadIdx.x & 63;
    // (a tick whose shards overflowed has gaps where runs were dropped: none of its frames leaves a list; in the heard form
    // neither does a tick whose heard links exceed the link capacity: its ordered records stop at `cap`)
    const bool dropped = t.stage_count[1] != 0u || (heard && t.out_count[1] != 0u);
    bool mine = false;
    int s = -1;
    uint32_t cnt = 0;
    // (heard: a listed frame has no hit, and neither has any frame of a tick without one)
    if (e < n_eval && !dropped && (heard || t.nc.hit[e].x == 0u)) {
        s = t.p_src[e];
        if (s >= 0) {
            bool won;
            if (heard) {
                // the pool's entry: "claimed in this epoch, not valid" keeps every context off the source, this one's later launch
                // sequences included, until k_nc_publish_batch stores the valid entry behind the fill
                const unsigned long long en = __hip_atomic_load(&t.nc.entry[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                won = (nc_entry_word(en) >> 1) != (t.nc.word >> 1) && atomicCAS(&t.nc.entry[s], en, (unsigned long long)nc_entry_pack(t.nc.word & ~1u, 0u, 0u)) == en;
            } else {
                const uint32_t st = t.nc.state[s];
                won = (st >> 1) != (t.nc.word >> 1) && atomicCAS(&t.nc.state[s], st, t.nc.word & ~1u) == st;
            }
            if (won) {
                cnt = heard ? t.cursor[e - t.cnt_base] : t.cand_tot[e - t.cnt_base]; // (heard: the frame's final heard count)
                mine = cnt <= kNcListCap;
            }
        }
    }
    // the wave's lists follow each other in the arena: one allocation per wave
    const uint32_t want = mine ? cnt : 0u;
    const uint32_t inc = wave_inclusive_scan(want, lane);
    const uint32_t wave_total = uint32_t(__shfl(int(inc), 63));
    unsigned long long o = 0;
    if (wave_total) {
        if (lane == 0) o = atomicAdd(heard ? t.nc.bump : &t.nc.ctr[0], (unsigned long long)wave_total);
        o = (unsigned long long)uint32_t(__shfl(int(uint32_t(o)), 0)) | ((unsigned long long)uint32_t(__shfl(int(uint32_t(o >> 32)), 0)) << 32);
        o += inc - want;
    }
    int32_t fill = -1;
    if (mine && o + cnt <= (unsigned long long)t.nc.arena_len) {
        if (heard) {
            // (nothing becomes valid here: the records are not in the arena yet, and another stream may look at any time)
            fill = cnt ? int32_t(o) : kNcFillEmpty;
        } else {
            t.nc.off[s] = uint32_t(o);
            t.nc.len[s] = cnt;
            t.nc.state[s] = t.nc.word; // (this thread owns the word; read by later launch sequences of this context only)
            if (cnt) fill = int32_t(o);
        }
    }
    if (k >= n_walk) return;
    t.nc.fill[k] = fill;
    if (!heard) t.nc.cur[e] = 0u; // (candidates copied so far: the heard form's fill does not count)
    // (heard form: the accepted lists without entries count as well -- a tick of nothing else still has them to publish; the fill
    // finds no record to copy for them)
    const uint64_t fm = ballot64(fill != -1);
    if (fm && int(threadIdx.x & 63) == __ffsll((long long)fm) - 1) atomicAdd(&t.nc.tick_cnt[1], uint32_t(__popcll(fm)));
}

// the entries of the lists claimed in this launch sequence (nothing to do for a tick that claimed none)
// Heard form: up to 64 positions per wave (list entries in a tick with hits, else frames).  A claimed frame's records are
// contiguous and already in node order at its place in the ordered arrays; all of the wave's lists are copied to the arena's
// columns with full lanes (no atomics; wave_copy_lists, rm_device.hpp).  A list's positions are dealt out evenly over ALL waves
// of the tick's grid: nearly every listed frame is claimed, and 64 of them to a wave left a tick with 28 % of its 1000 frames
// unserved to five waves of eleven dependent load -> store spans each, where sixteen waves had shared them before there was a
// list (this kernel's launches of such sequences, traced: 16-26 us before the list, 31-56 with 64 positions per wave).
// Candidates form: one workgroup per shard: the shard's entries (the sweep's: the cached ones are appended afterwards) whose
// frame fills a list go there, one atomic per run of entries of one frame.
// Measured and dropped: 2, 4 or 8 waves (gridDim.y) sharing the 64 frames' records, each taking every P-th span, as for
// k_reorder_served_batch (rm_reorder.hip; this kernel's total over a run, ms, two runs each of the default run | --warmup 24):
// 1 wave 0.32 0.35 | 0.35 0.36   2 waves 0.28 0.28 | 0.42 0.42   4 waves 0.32 0.36 | 0.37 0.37   8 waves 0.43 0.47 | 0.56 0.51 (one
// round per step, as before this loop: 0.43 0.46 | 0.49 0.48).  2 gain on one run what they lose on the other, 4 gain nothing.
__global__ void __launch_bounds__(256) k_nc_fill_batch(const TickDev *__restrict__ ticks)
{
    const TickDev &t = ticks[blockIdx.z];
    if (t.nc.state == nullptr || uniform_u(t.nc.tick_cnt[1]) == 0u) return;
    if (t.nc.arena_rssi != nullptr) { // (block-uniform; grid: frames / kBlock in x, 1 in y)
        // positions of the tick's list of frames without a hit where the tick has hits, else its frames -- as in the claim, which
        // wrote fill[] by the same positions.  `per` consecutive positions per wave: 64 of the frames, an even share of a list
        // (the grid has a wave per 64 frames of the largest tick, so a share is at most 64)
        const int n_eval = t.n_active - t.first_eval;
        const bool listed = uniform_u(t.nc.tick_cnt[2]) != 0u;
        const int n_walk = listed ? min(int(uniform_u(t.nc.tick_cnt[3])), n_eval) : n_eval;
        const int lane = threadIdx.x & 63;
        const int wave = int(blockIdx.x) * (kBlock / 64) + wave_index();
        const int n_waves = int(gridDim.x) * (kBlock / 64);
        const int per = listed ? min(64, (n_walk + n_waves - 1) / n_waves) : 64;
        const int e0 = wave * per;
        if (e0 >= n_walk) return; // (wave-uniform)
        const int k = e0 + lane;
        int32_t fo = -1;
        if (lane < per && k < n_walk) fo = t.nc.fill[k];
        int e = k;
        if (listed && fo >= 0) e = t.nc.unserved[k];
        // (claimed: the tick was not dropped, so every record of the frame lies below `cap`)
        const uint32_t cnt = fo >= 0 ? t.cursor[e - t.cnt_base] : 0u;
        const uint32_t inc = wave_inclusive_scan(cnt, lane);
        const uint32_t total = uniform_u(uint32_t(__shfl(int(inc), 63)));
        if (total == 0u) return; // (wave-uniform)
        const uint32_t src = fo >= 0 ? t.slot_off[e - t.cnt_base] : 0u;
        // (the claim has made sure of both ends -- the list ends inside the arena, the tick was not dropped; like the candidates
        // form's fill below, the copy guards them all the same: it writes into memory shared by every tick)
        wave_copy_lists<true>(t, lane, e0, cnt, inc, total, uint32_t(fo), src);
        return;
    }
    const uint32_t shard = blockIdx.y;
    if (shard > t.shard_mask || t.stage_count[1] != 0u) return;
    const uint32_t n = uniform_u(min(t.shard_count[shard * kShardStride], t.seg_cap));
    const int lane = threadIdx.x & 63;
    for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) { // block-uniform
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t idx = shard * t.seg_cap + i;
        int e = -1, fo = -1;
        if (i < n) {
            e = t.st_pkt[idx];
            fo = t.nc.fill[e];
        }
        const RunInfo ri = run_prefix(e, fo >= 0, lane);
        uint32_t base = 0;
        if (fo >= 0 && lane == ri.start) base = atomicAdd(&t.nc.cur[e], ri.total);
        base = uint32_t(__shfl(int(base), ri.start));
        if (fo >= 0) {
            const uint32_t k = uint32_t(fo) + base + ri.before;
            if (k < t.nc.arena_len) t.nc.arena[k] = t.st_dst[idx];
        }
    }
}

// heard form: the lists claimed in this launch sequence become valid -- a launch of its own behind the fill, so that the fill's
// records are written back before any entry says so.  One thread per position of the claim's walk: fill[k] tells an accepted
// list (its offset, or kNcFillEmpty) from a frame that claimed nothing; the entry -- valid bit, offset, length -- is one
// agent-scope store, which a pre-pass on another stream sees whole or not at all.  A tick that claimed nothing returns at once.
__global__ void __launch_bounds__(256) k_nc_publish_batch(const TickDev *__restrict__ ticks)
{
    const TickDev &t = ticks[blockIdx.z];
    if (t.nc.state == nullptr || t.nc.arena_rssi == nullptr || uniform_u(t.nc.tick_cnt[1]) == 0u) return;
    const int n_eval = t.n_active - t.first_eval;
    const bool listed = uniform_u(t.nc.tick_cnt[2]) != 0u;
    const int n_walk = listed ? min(int(uniform_u(t.nc.tick_cnt[3])), n_eval) : n_eval;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_walk) return;
    const int32_t fo = t.nc.fill[k];
    if (fo == -1) return;
    const int e = listed ? t.nc.unserved[k] : k;
    if (e < 0 || e >= n_eval) return;
    const int s = t.p_src[e];
    if (s < 0) return;
    // (an empty list lies nowhere: offset 0, so that the arena's very end needs no 28th bit)
    const uint32_t len = fo >= 0 ? t.cursor[e - t.cnt_base] : 0u;
    __hip_atomic_store(&t.nc.entry[s], (unsigned long long)nc_entry_pack(t.nc.word, fo >= 0 ? uint32_t(fo) : 0u, len), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what the frames that the pre-pass took out of the sweep get from their sources' lists
// Heard form: one thread per frame: the list's length goes into cursor[] -- the frame's heard count for the reorder stage's scan.
// Candidates form: one wave per 64 frames: the list of each hit frame goes into one of the tick's shards as a run of (frame,
// engine position) entries, all of the wave's lists copied with full lanes (an entry finds its frame by bisection over the lanes'
// running counts, wave_run_of), and every list's length into its frame's candidate count -- what the sweep would have appended
// (the order inside a shard never mattered: the reorder stage ranks by node index)
__global__ void __launch_bounds__(256) k_nc_expand_batch(const TickDev *__restrict__ ticks)
{
    const TickDev &t = ticks[blockIdx.z];
    if (t.nc.state == nullptr || uniform_u(t.nc.tick_cnt[2]) == 0u) return;
    const int lane = threadIdx.x & 63;
    const int e0 = int(blockIdx.x) * kBlock + wave_index() * 64;
    const int e = e0 + lane;
    uint2 h = make_uint2(0u, 0u);
    if (e < t.n_active - t.first_eval) h = t.nc.hit[e];
    uint32_t cnt = h.x > 1u ? h.x - 1u : 0u; // (0: swept, or an empty list)
    if (t.nc.arena_rssi != nullptr) {
        // heard form (block-uniform): the list IS the frame's heard links.  Its length joins the reorder stage's scan of cursor[]
        // (the pre-pass zeroed it; the exact stage adds to swept frames' words only); nothing goes to the shards, the frame's
        // candidate count stays 0 and the exact stage never sees it.
        if (cnt) t.cursor[e - t.cnt_base] = cnt;
        return;
    }
    // a list is one run in one shard (the sweep's runs are no longer: a shard has room for cap / shards entries)
    uint32_t dst = 0;
    if (cnt) {
        atomicAdd(&t.cand_tot[e - t.cnt_base], cnt);
        const uint32_t shard = (uint32_t(e) * 37u + uint32_t(blockIdx.z) * 101u) & t.shard_mask;
        const uint32_t base = atomicAdd(&t.shard_count[shard * kShardStride], cnt);
        if (base + cnt > t.seg_cap) { // the shard is full: drop the run, flag the tick
            t.stage_count[1] = 1u;
            cnt = 0u;
        }
        dst = shard * t.seg_cap + base;
    }
    const uint32_t inc = wave_inclusive_scan(cnt, lane);
    const uint32_t total = uniform_u(uint32_t(__shfl(int(inc), 63)));
    for (uint32_t j0 = 0; j0 < total; j0 += 64u) { // wave-uniform
        const uint32_t j = j0 + uint32_t(lane);
        const int f = wave_run_of(inc, j);
        const uint32_t f_inc = uint32_t(__shfl(int(inc), f)), f_cnt = uint32_t(__shfl(int(cnt), f)), f_off = uint32_t(__shfl(int(h.y), f));
        const uint32_t f_dst = uint32_t(__shfl(int(dst), f));
        if (j < total) {
            const uint32_t k = j - (f_inc - f_cnt);
            t.st_pkt[f_dst + k] = e0 + f;
            t.st_dst[f_dst + k] = t.nc.arena[f_off + k];
        }
    }
}

hipError_t launch_nbr_cache_batch(hipStream_t s, const TickDev *ticks, int n, const TickDev *b, bool behind_reorder)
{
    int max_eval = 0;
    uint32_t shards = 1;
    for (int i = 0; i < n; ++i) {
        max_eval = max(max_eval, ticks[i].n_active - ticks[i].first_eval);
        shards = max(shards, ticks[i].shard_mask + 1u);
    }
    if (max_eval <= 0) return hipSuccess;
    const bool heard = ticks[0].nc.arena_rssi != nullptr;
    if (heard && !behind_reorder) {
        RM_KLAUNCH(k_nc_expand_batch, dim3(cdiv(max_eval, kBlock), 1, n), dim3(kBlock), 0, s, b);
    } else if (heard) {
        RM_KLAUNCH(k_nc_claim_batch, dim3(cdiv(max_eval, 256), 1, n), dim3(256), 0, s, b);
        RM_KLAUNCH(k_nc_fill_batch, dim3(cdiv(max_eval, kBlock), 1, n), dim3(kBlock), 0, s, b);
        RM_KLAUNCH(k_nc_publish_batch, dim3(cdiv(max_eval, 256), 1, n), dim3(256), 0, s, b);
    } else if (!behind_reorder) {
        RM_KLAUNCH(k_nc_claim_batch, dim3(cdiv(max_eval, 256), 1, n), dim3(256), 0, s, b);
        RM_KLAUNCH(k_nc_fill_batch, dim3(1, shards, n), dim3(256), 0, s, b);
        RM_KLAUNCH(k_nc_expand_batch, dim3(cdiv(max_eval, kBlock), 1, n), dim3(kBlock), 0, s, b);
    }
    return hipGetLastError();
}

} // namespace rm
