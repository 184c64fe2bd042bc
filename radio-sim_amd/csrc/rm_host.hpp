// rm_host.hpp -- what the C-ABI translation units (rm_api_*.cpp) share: the context, its result slots, the
// helpers that plan and launch a tick.  Internal: not part of the boundary (include/radiomedium_hip.h).
//
// There is deliberately no CPU fallback anywhere behind this header: every evaluation goes through the gfx950
// kernels of rm_*.hip, and rm_create fails when no HIP device can be used.
//
// Reference paths: /root/reference/radio-medium/java/se/sics/emul8/radiomedium/.
#pragma once

#include "rm_engine.h"
#include "rm_evorder.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace rmh {

extern thread_local std::string g_err; // rm_last_error()
int fail(int code, const std::string &msg);

#define RM_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return rmh::fail(RM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

#define RM_TRY(call)                                                                                   \
    do {                                                                                               \
        int r_ = (call);                                                                               \
        if (r_ != RM_OK) return r_;                                                                    \
    } while (0)

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t want, bool keep = false, hipStream_t s = nullptr)
    {
        if (want <= n) return hipSuccess;
        size_t grow = std::max(want, n + n / 2);
        T *q = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&q), grow * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p && n) {
            e = hipMemcpyAsync(q, p, n * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(q);
                return e;
            }
        }
        if (p) (void)hipFree(p);
        p = q;
        n = grow;
        return hipSuccess;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

size_t pad64(size_t v);

// The pinned, host-mapped block a list call is staged through, counted in bytes, in ONE layout: n rows of row_bytes (records in or
// out), then one rm_stats_totals (out), then the node list (in).
struct PinnedBlock {
    char *p = nullptr;
    size_t bytes = 0;
    size_t o_totals = 0, o_nodes = 0; // where the last ensure laid the totals and the list
    std::vector<int32_t> last;        // (rows_write: by node index, the last list entry that names the node)
    // room for n rows of row_bytes, grown by half (at least 7 KiB: 256 entries of the smallest table's list update).  The stream
    // is idle when this returns, grown or not: no earlier list call's launch reads or writes the block, the caller may overwrite it
    int ensure(hipStream_t s, size_t n, size_t row_bytes)
    {
        RM_HIP(hipStreamSynchronize(s));
        o_totals = pad64(n * row_bytes);
        o_nodes = o_totals + pad64(sizeof(rm_stats_totals));
        const size_t need = o_nodes + pad64(n * 4);
        if (bytes >= need && p) return RM_OK;
        release();
        const size_t want = std::max<size_t>(need + need / 2, 256 * (sizeof(rm_listen_schedule) + 4));
        RM_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocMapped));
        bytes = want;
        return RM_OK;
    }
    char *rows() const { return p; }
    rm_stats_totals *totals() const { return reinterpret_cast<rm_stats_totals *>(p + o_totals); }
    int32_t *nodes() const { return reinterpret_cast<int32_t *>(p + o_nodes); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// The 64 pinned, host-mapped bytes through which a query's host loop reads a few device words between its launches (a queue's tail,
// a round's counter, the totals).
struct PinnedWords {
    unsigned long long *p = nullptr;
    hipError_t ensure() { return p ? hipSuccess : hipHostMalloc(reinterpret_cast<void **>(&p), 64, hipHostMallocMapped); }
    // bytes (<= 64) at dev_src as the launches enqueued on `s` so far leave them: one copy, one wait
    int read(hipStream_t s, const void *dev_src, size_t bytes)
    {
        RM_HIP(hipMemcpyAsync(p, dev_src, bytes, hipMemcpyDeviceToHost, s));
        RM_HIP(hipStreamSynchronize(s));
        return RM_OK;
    }
    uint32_t low() const { return uint32_t(p[0]); } // (a 4-byte read: the low half of the first word)
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
};

// what a pool of heard lists (rm_ncpool.hpp) owns on its device: one entry per node, the three columns of the arena, the arena's
// bump counter, and the event behind the last epoch's resets -- a context that joins makes its stream wait for it
struct NcPoolMem {
    DevBuf<unsigned long long> entry, bump;
    DevBuf<int32_t> arena;
    DevBuf<double> arena_rssi;
    DevBuf<uint8_t> arena_verdict;
    size_t arena_len = 0;
    hipEvent_t reset_ev = nullptr;
};
NcRegistry<NcPoolMem> &nc_registry();

} // namespace rmh

using rmh::DevBuf;
using rmh::PinnedBlock;

// Everything one evaluated tick owns on the device.  A context is its own slot 0; rm_batch_*
// adds further slots so that several ticks can be in flight through one launch sequence.
struct TickSlot {
    DevBuf<rm_tx_record> d_tx;   // records uploaded by the host / built from source indices
    DevBuf<float4> d_p_txf;      // per-frame pre-filter records
    DevBuf<int32_t> d_p_ch, d_p_src;
    DevBuf<float> d_p_inv;

    DevBuf<uint32_t> d_cnt, d_off, d_slot_tot, d_slot_off;
    // a rank's frame list (k_rank_frames): the listed frames' gathered-slot numbers, the listed frames before
    // every gathered slot, and the tick's LOCAL offsets (d_slot_off then holds the offsets by global packet number)
    DevBuf<int32_t> d_fl_map;
    DevBuf<uint32_t> d_fl_lb, d_slot_off_loc;
    DevBuf<unsigned long long> d_dense_mask; // the dense tick's heard links: 16 lane masks per (frame, chunk of 1024 nodes)

    DevBuf<uint32_t> d_counters; // two parities x 8: [1] dropped flag, [2..5] out_count
    DevBuf<uint32_t> d_shards;   // two parities x kShards x kShardStride append counters
    DevBuf<uint32_t> d_cursor, d_cand_tot, d_seg_off;
    DevBuf<int32_t> d_a_e;
    int zero_len = 0;        // slots of cursor / cand_tot that may be non-zero
    int parity = 0;
    DevBuf<int32_t> d_st_pkt, d_st_dst, d_st_next, d_head;
    DevBuf<uint32_t> d_st_blk;
    DevBuf<double> d_st_aux, d_st_lin, d_st_sinr, d_st_prob;
    DevBuf<int32_t> d_st_orig;
    DevBuf<uint8_t> d_st_flags, d_st_coll;
    DevBuf<int32_t> d_out_pkt, d_out_dst, d_a_pkt, d_a_dst;
    DevBuf<uint8_t> d_out_verdict, d_pkt_interf, d_a_verdict;
    DevBuf<double> d_out_rssi, d_out_sinr, d_out_prob, d_a_rssi, d_a_sinr, d_a_prob;
    DevBuf<uint32_t> d_draw_scan, d_scan_block;
    DevBuf<float4> d_scan_xyzr;  // the SINR medium's tick by scan: one record per frame on the air (TickDev::scan_xyzr / scan_ch) ...
    DevBuf<int32_t> d_scan_ch;
    DevBuf<uint32_t> d_sg_cnt, d_sg_every; // ... and the tick's index of them (ScanDev): counters in two parities, the cells' entries
    DevBuf<float4> d_sg_bxyzr;
    DevBuf<int2> d_sg_bci;
    DevBuf<int32_t> d_self_next;
    DevBuf<unsigned long long> d_self_slot; // per node; entries carry the tick's stamp (never cleared)
    int sg_parity = 0;
    bool sg_clean[2] = {false, false};      // the parity's counters are zero (the tick by scan before left them so)
    DevBuf<uint64_t> d_pkt_rng;
    DevBuf<uint32_t> d_pkt_draw_cnt, d_all_cnt;
    bool draws_pending = false; // partitioned + probabilistic: waiting for rm_tick_finish_draws
    rm::ModelDev pending_model{};
    uint32_t alloc_cap = 0;
    int alloc_feat = 0; // kFeat* buffers allocated at alloc_cap

    // last tick
    rm::TickDev last{};
    int last_n_new = 0;
    bool have_result = false;
    int64_t last_links = 0;
    // the closed-loop tick (rm_tick.hip) leaves per-frame ordered segments; the compact packet-major
    // arrays of rm_device_result are produced (k_reorder) when somebody asks for them
    bool compact_pending = false;
    // the dense tick (rm_dense.hip) leaves the heard links as lane masks per (frame, 1024 nodes) cell: the records are written
    // when somebody asks for them (materialize); rm_result_dense hands out the masks themselves
    bool dense_pending = false, dense_result = false;
    bool dense_listen = false; // the listening schedules' pass ran over this dense tick's records: the masks do not carry its verdicts
    bool dense_layout_pending = false; // ... and so are the cells' offsets and the totals (dense_layout)
    int dense_rx_first = 0, dense_chunks = 0;
    rm::ModelDev last_model{};
    rm::LaunchCfg last_cfg{};

    void release_all();
};

struct rm_context : TickSlot {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    rm_model_params params{};
    rm_error_model em{};       // the frame error model (E10); kind RM_EM_NONE: off
    // per-node traffic counters (E11; rm_api_stats.cpp, rm_stats.hip): the table by node index, the totals, and the pinned,
    // host-mapped block a list read is staged through (node list in; records and totals out)
    struct Stats {
        bool on = false;
        int32_t n = -1; // the node count the table was made (and zeroed) for; -1: never enabled
        DevBuf<rm_node_stats> table;
        DevBuf<rm_stats_totals> totals;
        PinnedBlock h;
    } st;
    // receiver listening schedules (E13; rm_api_listen.cpp, rm_listen.hip): one schedule and one missed count per node index, the
    // host's copy of the schedules (rm_listen_get reads it; a list update is applied to it in order), and the pinned, host-mapped
    // block a list update or a list read is staged through
    struct Listen {
        bool on = false;
        int32_t n = -1; // the node count the tables were made for; -1: never set (or cleared by another node count)
        std::vector<rm_listen_schedule> host;
        DevBuf<rm_listen_schedule> sched;
        DevBuf<uint64_t> missed;
        PinnedBlock h;
    } ls;
    // watched-link statistics (E14; rm_api_linkstats.cpp, rm_linkstats.hip): K peer slots and K entries per node index, the totals,
    // the host's copy of the peer rows (rm_linkstats_peers_get reads it), the device staging of a whole-table watch and the pinned,
    // host-mapped block a list watch or a list read is staged through
    struct LinkStats {
        int32_t K = 0;  // slots per node; 0: off
        int32_t n = -1; // the node count the tables were made for; -1: off
        std::vector<int32_t> host;
        DevBuf<int32_t> peer, stage;
        DevBuf<rm_link_stats> table;
        DevBuf<rm_stats_totals> totals;
        PinnedBlock h;
        // rm_linkstats_watch_device (rm_api_neighbors.cpp): the rows never pass through the host, so its copy is refreshed from the
        // device's table when somebody next reads it; the validation's per-node marks, its stamp and its pinned flag word
        bool host_stale = false;
        DevBuf<uint32_t> mark;
        uint32_t stamp = 0;
        uint32_t *h_bad = nullptr;
    } lk;
    // the neighbour query (E16; rm_api_neighbors.cpp, rm_neighbors.hip): what a RM_NB_HEARS query gathers from the table per call --
    // two words (the largest txpower, the number of radios that are off) and the list of those nodes
    struct Neighbors {
        DevBuf<unsigned long long> prep;
        DevBuf<int32_t> off_list;
    } nb;
    // the hop query (E17; rm_api_hops.cpp, rm_hops.hip): its own prep words and list of radios that are off (E16's are not
    // touched) -- words[0 .. 1] are k_nb_prep's, the low half of words[2] is the queue's tail; one 32-byte block, zeroed per
    // query --, the queue of labelled nodes ([n_nodes]: every level's frontier is a range of it), and the pinned words the
    // tail is read through once per level.  Nothing is allocated before the first query.
    struct Hops {
        DevBuf<unsigned long long> words;
        DevBuf<int32_t> off_list;
        DevBuf<int32_t> queue;
        rmh::PinnedWords h;
    } hp;
    // the route query (E18; rm_api_routes.cpp, rm_routes.hip): scratch of its own (the hop query's is not touched) -- words[0 .. 1]
    // are k_nb_prep's, words[2] the two queues' tails, words[3 .. 4] the totals' sums; one block, zeroed per query --, the list of
    // radios that are off, the per-node round stamps, the two frontier queues ([n_nodes] each), and the pinned words the tail
    // and the sums are read through.  Nothing is allocated before the first query.
    struct Routes {
        DevBuf<unsigned long long> words;
        DevBuf<int32_t> off_list;
        DevBuf<uint32_t> stamp;
        DevBuf<int32_t> queue; // [2][n_nodes]
        rmh::PinnedWords h;
        int32_t last_rounds = 0;   // the last query's relaxation launches and the frontier entries they walked (rm_routes_last_work)
        uint64_t last_entries = 0;
    } rt;
    // the measured-route query (E21; rm_api_etx.cpp, rm_etx.hip): every entry's link cost ([n_nodes][K]), the per-node round
    // stamps, the word block (rm::kEtxWords, zeroed per query) and the pinned words a round's counter and the totals are read
    // through.  Nothing is allocated before the first query.
    struct Etx {
        DevBuf<uint32_t> lc;
        DevBuf<uint32_t> stamp;
        DevBuf<unsigned long long> words;
        rmh::PinnedWords h;
        int32_t last_rounds = 0;    // the last query's relaxation launches and the nodes they examined (rm_etx_last_work)
        uint64_t last_examined = 0;
    } etx;
    // traffic schedules (E15; rm_api_traffic.cpp, rm_traffic.hip): one schedule per node index; the pinned, host-mapped block a list
    // update or a list read is staged through; the generator's scratch (the windows, the units' counts and packets) and the pinned
    // staging of its windows -- two blocks, each rewritten only after its copy has completed
    struct Traffic {
        bool on = false;
        int32_t n = -1; // the node count the table was made for; -1: never set (or cleared)
        DevBuf<rm_traffic_schedule> sched;
        PinnedBlock h;
        DevBuf<int64_t> d_win;
        DevBuf<int32_t> d_unit_count;
        DevBuf<uint64_t> d_unit_packets;
        int64_t *h_win[2] = {nullptr, nullptr};
        hipEvent_t h_ev[2] = {nullptr, nullptr};
        int gen = 0;
    } tf;
    // the unicast outcome query (E12; rm_api_unicast.cpp, rm_unicast.hip): what the last evaluating call left -- how many result slots,
    // and whether it was a gathered / rm_dist_* / rm_group_* form -- the slots' descriptors in device memory (rm::UcSlot per slot,
    // then the prefix of a slots-form query), their pinned staging (two blocks, each rewritten only after its copy has completed), and
    // the host forms' device scratch (lists in, outputs out)
    struct Unicast {
        int slots = 0; // 0: no evaluating call yet
        bool gathered = false;
        DevBuf<char> d_desc, d_io;
        char *h_desc[2] = {nullptr, nullptr};
        hipEvent_t h_ev[2] = {nullptr, nullptr};
        int gen = 0;
    } uc;
    // What a relay feature -- a node table driven by a finished result slot -- keeps whatever it relays (the relay_* helpers at the
    // end of this file work on it): the claim word per node every call leaves at rest, the source list's unit counts, the host
    // forms' lists in device memory, and the pinned, host-mapped block a list read is staged through.  Nothing is allocated
    // before the feature's enable.
    struct Relay {
        bool on = false;
        int32_t n = -1; // the node count the tables were made for; -1: off
        DevBuf<int32_t> claim, unit_count, stage;
        PinnedBlock h;
    };
    // forwarding queues (E19; rm_api_fwd.cpp, rm_fwd.hip): the parameters, the tables by node index (the rows, the packets
    // [n][queue_slots], the totals), the rest of the per-node scratch, the per-packet-number records of an advance or an inject
    struct Fwd : Relay {
        rm_fwd_params p{};
        DevBuf<rm_fwd_node> node;
        DevBuf<rm_fwd_packet> pk;
        DevBuf<rm_fwd_totals> totals;
        DevBuf<int32_t> acc, pushed;
        DevBuf<rm::FwdAct> act;
    } fw;
    // dissemination floods (E20; rm_api_flood.cpp, rm_flood.hip): the parameters, the table by node index and its totals, the
    // rest of the per-node scratch, one word per entry of an advance or seed list
    struct Flood : Relay {
        rm_flood_params p{};
        DevBuf<rm_flood_node> node;
        DevBuf<rm_flood_totals> totals;
        DevBuf<int32_t> pmin, act;
        DevBuf<int64_t> tmin;
    } fl;
    // neighbour tables (E22; rm_api_nbtable.cpp, rm_nbtable.hip): the parameters, the counters by node index and their totals, one
    // word of scratch per node.  The peers and entries it writes are the watched-link statistics' (lk); of the base it uses the
    // staging of a host pin array and the block of a list read, never the claim words or the unit counts
    struct NbTable : Relay {
        rm_nbtable_params p{};
        DevBuf<rm_nbtable_node> node;
        DevBuf<rm_nbtable_totals> totals;
        DevBuf<uint64_t> bid;
    } nt;
    // link estimator (E23; rm_api_linkest.cpp, rm_linkest.hip): K, the parameters, the entries and the published table
    // ([n_nodes][K] each), the node state, the totals, and the device copies of a host fold's inputs.  The tables it reads are the
    // watched-link statistics' (lk) and the forwarding queues' (fw), or the caller's; of the base it uses the block of a list read
    struct LinkEst : Relay {
        int32_t K = 0;
        rm_linkest_params p{};
        DevBuf<rm_linkest_entry> entry;
        DevBuf<rm_linkest_node> node;
        DevBuf<int32_t> pub_peer;
        DevBuf<rm_link_stats> pub_stats;
        DevBuf<rm_linkest_totals> totals;
        DevBuf<int32_t> in_peer;
        DevBuf<rm_link_stats> in_stats;
        DevBuf<rm_fwd_node> in_fwd;
    } le;
    double base_rssi = -100.0; // AbstractRadioMedium.java:38

    // host mirror of the node table (Simulator.getNodes() snapshot)
    int n = 0;
    std::vector<double> x, y, z, txpower, rxprob, txprob;
    std::vector<int32_t> channel, int_id;
    std::vector<uint8_t> enabled;
    // device-resident source table (SoA, node-index order): what a packet copies from its source
    DevBuf<double> d_x, d_y, d_z, d_txpower, d_txprob, d_rxprob_node;
    DevBuf<int32_t> d_channel, d_int_id;
    DevBuf<rm::SrcRecord> d_srec; // ... and the same as one 64-byte record per node (what a packet copies from its source)
    // device-resident receiver table of this partition (SoA, engine order = spatially sorted)
    DevBuf<double> d_rx_x, d_rx_y, d_rx_z, d_rx_rxprob;
    DevBuf<int32_t> d_rx_channel, d_rx_int_id, d_rx_orig, d_pos_of;
    DevBuf<uint8_t> d_rx_enabled;
    DevBuf<rm::RxRecord> d_rx_rec;
    DevBuf<rm::RxCompact> d_rx_rec32;
    DevBuf<float4> d_rxf, d_bbox_xy, d_wg_box_xy;
    DevBuf<uint32_t> d_grp_chmask, d_wg_chmask;
    DevBuf<float2> d_wg_box_z;
    DevBuf<float2> d_bbox_z;
    DevBuf<double> d_n2n;
    int n2n_m = 0;
    DevBuf<uint32_t> d_shadow_tbl;
    bool shadow_tbl_valid = false;
    int n_rx = 0;            // receivers in the table
    bool rx_sorted = false;  // engine order != node-index order
    // changed nodes are written in place while the engine order is still a good spatial order
    struct GroupBox {
        double lo[3], hi[3];
    };
    std::vector<int32_t> h_pos_of;  // node index - pos_first -> engine position, -1 = no receiver here (host copy of d_pos_of)
    std::vector<GroupBox> g_box;    // per group of 64: its box when the table was sorted
    std::vector<uint8_t> g_escaped; // bit 0 / 1: a receiver of this group has left the box by more than 1/8 / 1/2 of its extent
    int drifted_groups = 0, escaped_groups = 0;
    int64_t table_sorts = 0;        // times the receiver table was (re)built
    DevBuf<rm::NodePatch> d_patch;

    // reception stage (rm_events.hip): pending packets + their links, radio state per node, delivery list block
    struct Events {
        bool on = false;
        uint32_t pk_cap = 0, pool_cap = 0, g_cap = 0;
        DevBuf<rm::EvState> d_st;
        DevBuf<rm::EvPacket> d_pk;
        DevBuf<int32_t> d_ldst;
        DevBuf<double> d_lrssi;
        DevBuf<uint8_t> d_lverdict;
        DevBuf<int64_t> d_gtime;
        DevBuf<uint64_t> d_gmeta;
        DevBuf<uint32_t> d_gref, d_grank, d_cnt, d_off, d_grun;
        DevBuf<unsigned long long> d_run_rec;
        DevBuf<unsigned long long> d_recv_key, d_send_key;
        DevBuf<uint8_t> d_receiving, d_sending;
        DevBuf<double> d_latched;
        int state_n = 0;          // nodes the radio-state arrays hold
        char *h_out = nullptr;    // host-mapped: EvHeader + packet / dst / rssi arrays of pool_cap entries
        char *h_info = nullptr;   // host-mapped: node-info answers
        int info_n = 0;
        uint32_t seq = 0, info_seq = 0;
        DevBuf<int32_t> d_info_nodes;
        // rm_node_info_changed: what was reported last per node, the kernel's counters, the host-mapped block of the changes
        DevBuf<double> d_rep_rssi;
        DevBuf<int2> d_rep_sc;
        DevBuf<uint32_t> d_rep_cnt;
        int rep_n = 0;            // nodes the report arrays hold (all "never reported" when (re)allocated)
        char *h_changed = nullptr;
        int changed_n = 0;
        uint32_t changed_seq = 0;
        int64_t next_packet = 0;  // host mirror of EvTails::gseq_next
        int64_t oldest_packet = 0; // number of the oldest pending packet as the last drain published it (a bound on the ring window)
        int par = 0;              // which EvState::tails are current (flips with every appended tick)
        // the tick evaluated last, not handed to the rings yet: a drain that follows at once takes it along (append + selection in
        // one launch, rm_events.hip); anything else that comes first -- another tick above all -- appends it on its own
        struct Pending {
            bool on = false;
            rm::EvLinkSrc ls{};
            const rm_tx_record *tx = nullptr;
            int n_new = 0, immediate = 0;
            int64_t now = 0;
            const uint32_t *dropped = nullptr;
        } pending;
        // rm_events_process_batch: the ticks of the last rm_batch_run_* that may still be handed over (0: none), and the
        // generation they were left in -- `gen` moves with whatever rewrites the slots, the node table or the medium, and with
        // every drain (ev_touch), so a batch whose slots are no longer what it evaluated is refused
        uint64_t gen = 0, batch_gen = 0;
        int batch_n = 0;
        bool batch_ok = false;    // ... and whether its form is one the hand-over takes (not the gathered / rm_dist_* forms)
        char *h_batch = nullptr;  // host-mapped: the batch's per-tick headers, then its runs and deliveries (grows geometrically)
        size_t h_batch_bytes = 0;
        rm::EvBatchSlot *h_bslots = nullptr; // pinned, host-mapped: [RM_MAX_BATCH] what k_ev_batch_size reads of the slots ...
        uint32_t *h_bsize = nullptr;         // ... and what it writes: pending links, pending packets, then per slot its links
    } ev;
    DevBuf<uint8_t> d_enabled;   // Transciever.isEnabled by node index

    int frac_probs = -1;         // cached: any rx/tx probability strictly between 0 and 1 (-1 = unknown)
    bool tick_frac_records = false; // a host record of the running tick has 0 < txprob < 1 (rm_enqueue_tx_records)
    bool rx_dirty = true;        // receiver table has to be rebuilt (positions / partition / model class)
    bool prefilter_dirty = true; // pre-filter records have to be recomputed
    double org[3] = {0, 0, 0};
    double coord_bound = 0, f32_slack = 0;

    int rx_first = 0, rx_count = -1; // receiver partition by index range (rm_set_partition); -1 = all nodes
    // receiver partition by region (rm_set_partition_spatial): region sp_part of sp_parts of the k-d split over ALL nodes;
    // sp_parts == 0: none.  The member nodes are fixed when the partition is set / the table is uploaded: a node that moves
    // stays with its rank (no other rank could learn that it left).
    int sp_part = 0, sp_parts = 0;
    std::vector<int32_t> sp_nodes;   // the region's nodes, ascending
    DevBuf<uint8_t> d_member;        // [n] 1 = a receiver of this context (spatial partitions; the reception stage's "owned")
    DevBuf<int32_t> d_draw_nodes;    // spatial partitions whose links draw: node index of every drawing link, packet-major
    DevBuf<uint32_t> d_all_off;      // [world][n_new] scratch of rm_tick_finish_draws_nodes
    DevBuf<int32_t> d_all_nodes;     // its host lists, uploaded
    // RCCL inside the library (rm_comm_*, rm_dist_*; rm_api_comm.cpp): this context's rank of a communicator
    void *comm = nullptr;            // ncclComm_t
    bool comm_owned = false;
    int comm_world = 1, comm_rank = 0;
    DevBuf<rm_tx_record> d_dist_mine, d_dist_all; // this rank's packed frames / the frames of all ranks [rank][tick][slot]
    DevBuf<int32_t> d_dist_idx;                   // the gathered source indices [rank][tick][slot] (what crosses the links)
    uint32_t cap = 1u << 22;
    int last_tile_reuse = 1; // ticks of the last batch a filter workgroup swept with one load of its receivers (rm_batch_tile_reuse)
    // Digest of the node table (rm_table_digest): xor over the nodes of a 64-bit hash of (index, every field), mixed with the node
    // count -- a function of the table's CONTENT, whatever sequence of uploads and updates produced it.  Ranks that exchange
    // source indices build each other's records from their own copies of the table: the digests ride in the all-gather and a
    // rank whose copy differs is found out (rm_dist_batch_run_sources_device, rm_batch_run_gathered_blocks_device).
    uint64_t table_xor = 0, table_digest = 0;
    DevBuf<int32_t> d_dist_stage; // this rank's block of a sharded batch: its source indices, then the trailer with the digest

    int64_t current_time = 0;
    int64_t t_begin = 0, t_end = 0;
    bool in_tick = false;

    // on-air list (host-record mode)
    std::vector<rm_tx_record> pending; // frames enqueued in the current tick
    // on-air list (device-source mode, SINR): the live batches are a window [air_head, air_tail) of
    // d_air; a batch = the frames of one rm_tick_run_sources_device call (same start and air time)
    struct AirBatch {
        int count;
        int64_t end_us;
        uint32_t tick; // AirLists::tick of the call that put the batch on the air
    };
    // the window holds frames that were selected for this partition's region (k_rank_frames over a batch of overlapping SINR ticks:
    // rm::CullEntry): the boxes the selections were made against, and until when each matters
    bool air_culled = false;
    DevBuf<rm::CullEntry> d_cull_ring;
    int64_t cull_end[rm::kCullRing] = {};
    uint32_t cull_seq = 0;
    DevBuf<rm_tx_record> d_air, d_air_alt; // (the window's buffer and the one it slides into when this one is used up: air_window_reserve)
    std::vector<AirBatch> air_batches;
    size_t air_head = 0, air_tail = 0;
    // the per-receiver interferer lists of the frames on the air, alive on the device from tick to tick (rm::AirDev):
    // a SINR tick evaluates its new frames only, as long as nothing the old entries were computed from has changed
    struct AirLists {
        DevBuf<rm::AirEntry> pool;
        DevBuf<unsigned long long> head;
        DevBuf<uint32_t> tail, mark, bad;
        bool valid = false;       // the lists hold exactly the frames on the air
        uint32_t tick = 0;        // number of the last tick that added entries (1 ..)
        uint32_t sub_cap = 0;     // entries per sub-ring (a power of two)
        int64_t last_t_begin = 0;
        uint64_t rebuilds = 0, incremental = 0;
        uint64_t scans = 0;       // ticks evaluated by scan (rm_airscan.hip): they leave nothing in the lists
        uint32_t stamp = 0;       // of the nodes' chains of own frames (TickSlot::d_self_slot of the context): one per tick by scan / per batch of overlapping ticks
    } air;
    int64_t air_max_t_begin = INT64_MIN; // the latest t_begin a tick over the on-air window has had (air_tick_device)
    // a batch of SINR ticks whose frames outlive their tick (rm_airbatch.hip, rm_api_airbatch.cpp): the batch's index of
    // the frames it can see, the surviving (link, frame) pairs, the descriptors' pinned staging
    struct Overlap {
        DevBuf<float4> fr_f, e_f;
        DevBuf<int4> fr_m, e_m;
        DevBuf<longlong2> fr_t, e_t;
        DevBuf<uint32_t> fr_bin, bin_cnt, bin_off, block_sum, every, misc, pair_tail, items;
        DevBuf<int32_t> self_next, slot_first;
        DevBuf<uint8_t> defer;
        DevBuf<rm::OvTick> ticks;
        DevBuf<rm::OvPair> pairs;
        size_t pair_cap = 0;        // entries over all shards
        size_t pair_cap_forced = 0; // RM_OV_PAIR_CAP (tests)
        char *h_desc[2] = {nullptr, nullptr}; // pinned: OvTick[RM_MAX_BATCH] then slot_first
        size_t h_desc_bytes[2] = {0, 0};
        hipEvent_t h_ev[2] = {nullptr, nullptr};
        int gen = 0;
        uint32_t *h_flag = nullptr; // pinned, one word per generation: OvDev::misc[1] of the batch that used the generation last (frames
                                    // were deferred, the pair list was full: grown for the next batch of that generation); read only
                                    // after that batch's copy has landed (h_flag_ev)
        hipEvent_t h_flag_ev[2] = {nullptr, nullptr};
        bool h_flag_used[2] = {false, false};
        uint64_t batches = 0, ticks_done = 0, last_frames = 0;
    } ov;
    // the channel energy query (rm_api_energy.cpp, rm_energy.hip): its index of the live frames, built from scratch per query, the
    // nodes' transmitting stamps, and the host form's pinned, host-mapped block (node list in, energies and flags out)
    struct Energy {
        DevBuf<uint32_t> cnt, tx_mark;
        DevBuf<int32_t> gated; // a gated tick's source list after the gate (rm_api_cca.cpp): the caller's list is never written
        DevBuf<float4> bucket_f, every_f;
        DevBuf<int4> bucket_m, every_m;
        uint32_t stamp = 0;
        char *h_block = nullptr;
        size_t h_cap = 0; // nodes the block has room for
        // the gate of a gated batch (rm_api_cca.cpp, rm_ccabatch.hip; rm::CcaBatchDev): its own index (every frame of the window and of the
        // batch), the candidates' records as if kept, their pair segments; `gated` holds the gated lists of all ticks, one after the other
        struct Batch {
            DevBuf<rm::CcaTick> ticks;
            DevBuf<rm_tx_record> scr;
            DevBuf<int32_t> cand, fr_tick, self_next, bucket_t, every_t;
            DevBuf<uint32_t> cnt, pair_cnt, pair_off, pair_fill, pair_slot;
            DevBuf<float4> bucket_f, every_f;
            DevBuf<int4> bucket_m, every_m;
            DevBuf<ulonglong2> pair_term, base;
            DevBuf<unsigned long long> pair_base;
            DevBuf<uint8_t> base_flags, kept;
            char *h_desc = nullptr; // pinned, host-mapped: CcaTick[RM_MAX_BATCH], then the words the device hands back (CcaBatchDev::h_info),
            size_t h_desc_extra = 0; // then this many bytes a CSMA-CA batch uploads its schedule from (cca_desc_block)
            void release_all()
            {
                ticks.release(); scr.release(); cand.release(); fr_tick.release(); self_next.release(); bucket_t.release(); every_t.release();
                cnt.release(); pair_cnt.release(); pair_off.release(); pair_fill.release(); pair_slot.release(); bucket_f.release();
                every_f.release(); bucket_m.release(); every_m.release(); pair_term.release(); base.release(); pair_base.release(); base_flags.release(); kept.release();
                if (h_desc) (void)hipHostFree(h_desc);
                h_desc = nullptr;
                h_desc_extra = 0;
            }
        } cb;
        // what a CSMA-CA gated batch adds to it (rm_api_csma.cpp, rm_csma.hip; rm::CsmaDev): the schedule on the device, the packets'
        // states, the slots' tentative bits; the host form's outputs before they are copied out
        // (E9: the carried packets' outputs of the host form; the carry-out's inputs on the device, its workgroup counts, and the pinned,
        // host-mapped block k_csma_collect writes the count and the records to)
        struct Csma {
            DevBuf<char> sched, collect_in;
            DevBuf<uint8_t> state, tentative, slot_flags, o_status, o_attempts, o_flags, c_status, c_attempts, c_flags;
            DevBuf<int32_t> o_tick, o_pkt, c_tick, c_pkt;
            DevBuf<double> o_energy, c_energy;
            DevBuf<uint32_t> collect_cnt;
            char *h_collect = nullptr; // pinned: the upload's staging ([0, h_collect_in)), the count (64 bytes), the carry-out's records
            size_t h_collect_in = 0, h_collect_out = 0;
            void release_all()
            {
                sched.release(); state.release(); tentative.release(); slot_flags.release(); o_status.release(); o_attempts.release();
                o_flags.release(); o_tick.release(); o_pkt.release(); o_energy.release();
                collect_in.release(); c_status.release(); c_attempts.release(); c_flags.release(); c_tick.release(); c_pkt.release();
                c_energy.release(); collect_cnt.release();
                if (h_collect) (void)hipHostFree(h_collect);
                h_collect = nullptr;
                h_collect_in = h_collect_out = 0;
            }
        } cs;
    } ed;
    bool dev_records_from_caller = false; // the tick being prepared takes rm_tx_record arrays the caller built in device memory
    mutable rm::ModelDev mdev{};            // model_dev()'s last answer and what it was derived from
    mutable unsigned char mdev_key[320] = {};
    mutable bool mdev_valid = false;

    DevBuf<uint64_t> d_rng;  // [1] java.util.Random state, shared by all slots
    rm::TransmitResult *h_transmit = nullptr; // host-mapped result block of rm_transmit
    // host-mapped result block of rm_tick_flush*: the last kernel of a flushed tick writes header,
    // offsets and records there, the host waits for the header's sequence number
    char *h_stage = nullptr;
    uint32_t stage_links = 0, stage_packets = 0, stage_seq = 0;
    DevBuf<uint32_t> d_pack_done;
    DevBuf<rm::PackSlot> d_pack;    // descriptors of rm_batch_result_view
    rm::PackSlot *h_pack = nullptr; // their pinned staging
    // pinned staging of the Tx records of rm_tick_begin / rm_enqueue_tx* (two buffers, each guarded by an event)
    rm_tx_record *h_tx[2] = {nullptr, nullptr};
    size_t h_tx_n[2] = {0, 0};
    hipEvent_t h_tx_ev[2] = {nullptr, nullptr};
    int h_tx_gen = 0;
    const rm_tx_record *host_src = nullptr; // the tick being prepared reads its records from this host-mapped block (prepare_tick)
    uint32_t transmit_seq = 0;
    DevBuf<rm::TickDev> d_ticks; // [RM_MAX_BATCH] descriptors of the running rm_batch_* call
    DevBuf<int32_t> d_near_list;  // [ticks][blocks of kNearSb filter workgroups][frames] near-frame lists of a batch over a large table
    DevBuf<uint32_t> d_near_cnt;  // [ticks][blocks]
    // the source candidate cache of the batched sweep (rm::NbrCacheDev): per node a state word and its list's place
    // in the arena; per tick of the running batch its counters and per-frame words.  `change` moves (prepare_nodes) whenever the
    // receiver table or the pre-filter is rebuilt; a batch that finds it moved begins a new epoch on the device: every list is
    // stale, the arena is handed out from its start again.  So does a batch of the candidates FORM behind one of the heard form
    // (heard: draw-free batches keep finished records; candidates otherwise).
    // The heard form's per-source part -- entries, arena columns, bump counter -- is not the context's: it lies in a pool
    // (rmh::NcPoolMem, rm_ncpool.hpp) shared with every context of the device whose table and medium are equal, attached to by
    // the first heard-form batch and left in rm_destroy.  `pool_seen` is the value of `change` the attachment was made or last
    // confirmed at.  The candidates form below stays private: its lists hold engine positions.
    struct NbrCache {
        DevBuf<uint32_t> state, off, len, tick_cnt, cur;
        DevBuf<int32_t> arena, fill, unserved;   // (arena, off, len: allocated by the first batch of the candidates form)
        DevBuf<uint2> hit;
        DevBuf<unsigned long long> ctr;
        uint64_t change = 1, seen = 0, pool_seen = 0;
        uint32_t epoch = 0;
        int nodes = -1;
        int form = -1;                 // of the last batch: 0 candidates, 1 heard
        unsigned long long batches[2] = {0, 0}; // launch sequences per form (nbr_cache_report)
        rmh::NcPool<rmh::NcPoolMem> *pool = nullptr;
    } nc;
    // larger batches: k_fetch_ticks reads them from pinned, host-mapped memory (two staging buffers, each
    // guarded by an event: it is rewritten only after the kernel that read it has completed)
    rm::TickDev *h_ticks[2] = {nullptr, nullptr};
    hipEvent_t h_ticks_ev[2] = {nullptr, nullptr};
    int h_ticks_gen = 0;
    std::vector<std::unique_ptr<TickSlot>> extra_slots; // result slots 1.. of rm_batch_*

    // instantiated hipGraphs of the per-tick launch sequence, keyed by a hash of every launch argument
    struct GraphEntry {
        uint64_t key;
        hipGraphExec_t exec;
        uint64_t last_use;
    };
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    bool use_graphs = false; // RM_GRAPH=1: replay the tick from a cached hipGraph (measured slower than eager
                             // launches on ROCm 7.2 for this 5-kernel sequence: 50 vs 46 us per tick)

    // profiling (rm_profile_enable): on every n-th launch sequence each kernel launch carries its own pair of events
    // (rm::KernelProbe); the intervals are summed per stage and per kernel
    bool profile = false;   // sampling on
    int profile_every = 1;  // sample every n-th launch sequence
    uint64_t tick_index = 0;
    struct Sample {
        struct K {
            hipEvent_t a = nullptr, b = nullptr;
            int stage = 0;
            const char *name = nullptr;
        };
        std::vector<K> k;   // (events are created once and reused)
        int n = 0;          // launches probed in this sample
        int cur_stage = 0;  // stage the launches being issued belong to
    };
    std::deque<Sample> ev_pool;
    size_t ev_used = 0;
    uint32_t prof_samples = 0;
    double prof_ms[RM_PROFILE_STAGES] = {0};
    struct KernelTime {
        std::string name;
        int stage;
        uint32_t launches;
        double ms;
    };
    std::vector<KernelTime> prof_kernels;
};

namespace rmh {

// ---- rm_api_context.cpp: model, derived constants
const char *model_name(int kind);
bool is_sinr(const rm_context *c);
int part_first(const rm_context *c); // first node index the position map covers
int part_count(const rm_context *c); // receivers of this context
int pos_span(const rm_context *c);   // node indices the position map covers (index partition: its nodes; spatial: all)
bool part_spatial(const rm_context *c);
bool frac(double p);
bool maybe_draws(rm_context *c);
int validate_model(const rm_model_params *p);
void recompute_frame(rm_context *c);
rm::ModelDev model_dev(const rm_context *c);
rm::NodesDev nodes_dev(rm_context *c);
bool is_geometric(const rm_context *c);
int build_shadow_table(rm_context *c);

// ---- rm_api_nodes.cpp: the receiver table
int rebuild_receivers(rm_context *c);
int select_region(rm_context *c);    // the member nodes of a spatial partition from the current node table
int patch_nodes(rm_context *c, const int32_t *nodes, int count);
int prepare_nodes(rm_context *c);

template <typename T> int upload(DevBuf<T> &d, const std::vector<T> &h, hipStream_t s)
{
    RM_HIP(d.ensure(std::max<size_t>(h.size(), 1)));
    if (!h.empty()) RM_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return RM_OK;
}

// ---- rm_api_plan.cpp: one tick's buffers, descriptor and launch sequence
// Link-sized buffers of a result slot.  Only what the configuration touches is allocated (a
// batch keeps up to RM_MAX_BATCH slots): `payload` = per-entry rssi / probability / node index
// (unsorted tables and SINR), `sinr` = per-receiver lists and linear powers, `draws` = the
// java.util.Random scan and the probabilities carried to it.
enum { kFeatPayload = 1, kFeatSinr = 2, kFeatDraws = 4 };
int ensure_link_buffers(rm_context *c, TickSlot &ts, int feat);

// What one tick's launch sequence needs besides the slot: filled by prepare_tick.
struct TickPlan {
    rm::TickDev t{};
    rm::ScanDev scan{};  // (t.air_scan only)
    rm::LaunchCfg cfg{};
    bool sinr = false, stochastic = false, partitioned = false;
    bool empty = false; // nothing to sweep: the result is an empty one
};

// A batch that plans its ticks and then returns without launching them hands the slots' counter parity back.  prepare_tick
// flips a slot to the other parity because the tick's first kernel zeroes the other parity's counters for the tick after it; a
// tick that is never launched zeroed nothing, and the next tick through the sweep kernels would start from the counters of the
// tick before last.  planned(): one more slot was flipped (a non-empty plan); dismiss(): the ticks are launched from here on.
struct ParityGuard {
    TickSlot *const *slots;
    const TickPlan *plans;
    int n = 0;
    bool armed = true;
    ParityGuard(TickSlot *const *s, const TickPlan *p) : slots(s), plans(p) {}
    void planned() { ++n; }
    void dismiss() { armed = false; }
    ~ParityGuard()
    {
        if (!armed) return;
        for (int b = 0; b < n; ++b)
            if (!plans[b].empty) slots[b]->parity ^= 1;
    }
    ParityGuard(const ParityGuard &) = delete;
    ParityGuard &operator=(const ParityGuard &) = delete;
};

// Buffers and descriptor of one tick in result slot `ts`; `tx` is the on-air list in device memory
// (build mode: where the records of the source indices `src_list` are written).
// kAirScan: `tx` holds every frame on the air (as for a rebuild), only the new ones are evaluated, their interferers are found
// among the frames themselves (rm_airscan.hip); the lists are not touched and count as stale afterwards
// kAirBatch: a tick of a batch of overlapping SINR ticks (rm_api_airbatch.cpp): swept as the medium without SINR (heard links
// only, cut-off at the sensitivity); the interference stages of the whole batch follow the sweep
enum { kAirNone = 0, kAirIncremental = 1, kAirRebuild = 2, kAirScan = 3, kAirBatch = 4 };
bool air_scan_applies(rm_context *c, int n_new); // (after prepare_nodes)
uint32_t air_sub_cap(const rm_context *c);
bool air_lists_current(const rm_context *c, int64_t t_begin, uint32_t oldest);
int prepare_tick(rm_context *c, TickSlot &ts, TickPlan &plan, bool want_wg, const rm_tx_record *tx, int n_active,
                 int first_new, const int32_t *src_list = nullptr, int64_t src_start_us = 0, int64_t src_air_us = 0,
                 int air_mode = kAirNone, uint32_t air_oldest = 0, const rm::PlanKnobs *knobs_in = nullptr);
// em_pass: with the frame error model on, the tick ends with its compact arrays and the model's pass over them (a batch that
// launches its ticks one by one runs ONE pass over all of them afterwards instead); the same holds for the listening schedules'
// and the traffic counters' passes
int launch_tick(rm_context *c, TickSlot &ts, const TickPlan &plan, bool em_pass = true);
int materialize(rm_context *c, TickSlot &ts);
int dense_layout(rm_context *c, TickSlot &ts); // (the cells' offsets and totals of a dense tick that ended with its cells)
int run_tick(rm_context *c, const rm_tx_record *tx, int n_active, int first_new, const int32_t *src_list = nullptr,
             int64_t src_start_us = 0, int64_t src_air_us = 0, int air_mode = kAirNone, uint32_t air_oldest = 0, bool ev_may_wait = false);
int drain_profile(rm_context *c);
// a sampled launch sequence: begin_sample() returns the sample (or nullptr: not sampled) and routes the kernel probes of
// this thread to it; sample_stage() names the stage of the launches that follow; end_sample() unroutes.  (ProbeScope
// does the last two on every way out of a launch function.)
rm_context::Sample *begin_sample(rm_context *c);
inline void sample_stage(rm_context::Sample *smp, int stage) { if (smp) smp->cur_stage = stage; }
void end_sample();
struct ProbeScope {
    rm_context::Sample *smp;
    explicit ProbeScope(rm_context *c) : smp(begin_sample(c)) {}
    ~ProbeScope() { if (smp) end_sample(); }
    ProbeScope(const ProbeScope &) = delete;
    ProbeScope &operator=(const ProbeScope &) = delete;
};
// The same for a call that is no tick (a query, a gate, a generate, a drain, a relay feature's call): rm_profile_kernels names
// its kernels.  begin_sample (rm_api_plan.cpp) moves one piece of state that belongs to the ticks: it counts the launch sequence
// in c->tick_index, which decides which sequences are sampled under rm_profile_enable(every_n).  Such a call puts the count
// back: it is sampled iff the tick after it would be, and the ticks' sampling is as without the call
struct CallProbe {
    rm_context::Sample *smp;
    explicit CallProbe(rm_context *c)
    {
        const uint64_t tick_index = c->tick_index;
        smp = begin_sample(c);
        c->tick_index = tick_index;
    }
    ~CallProbe() { if (smp) end_sample(); }
    CallProbe(const CallProbe &) = delete;
    CallProbe &operator=(const CallProbe &) = delete;
};

// ---- rm_api_events.cpp: the reception stage
rm::EvDev ev_dev(rm_context *c);
int ev_ensure_nodes(rm_context *c);
int ev_append(rm_context *c, TickSlot &ts, bool may_wait = false);
inline void ev_touch(rm_context *c) { ++c->ev.gen; } // the slots / node table / medium changed, or a drain ran
void ev_batch_ran(rm_context *c, int rc, int n_ticks, bool eligible); // after rm_batch_run_*: what rm_events_process_batch may take
int ev_flush_append(rm_context *c);

// ---- rm_api_tick.cpp: results of an evaluated tick, the host-mapped result block
rm_tx_record make_record(const rm_context *c, int32_t src, int64_t start_us, int64_t air_us, const double *txpower,
                         const int32_t *channel);
const char *record_flag_message(uint32_t flag);
int copy_out(rm_context *c, TickSlot &ts, int32_t *pkt, int32_t *dst, uint8_t *verdict, double *rssi, double *sinr,
             uint32_t cap, uint32_t *count, uint8_t *pkt_interference, uint32_t *pkt_offset);
size_t pad64(size_t v);
rm::HostView stage_view(char *base, uint32_t links, uint32_t packets, size_t *bytes);
rm::BatchCounts *stage_counts(char *base);
int ensure_stage(rm_context *c, uint32_t links, uint32_t packets);
int pack_to_stage(rm_context *c, TickSlot &ts, rm::HostView *view);
// does this slot's result go to the host with ONE rssi per packet?  The reference's media hand the packet's transmit power to
// every heard link unchanged; the log-distance medium computes a link's own (RM_HOST_LINK_RSSI=1 keeps the column for all)
bool host_pkt_rssi(const rm_context *c, const TickSlot &ts);
int stage_status(rm_context *c, const rm::HostView &v);
int tick_run_host(rm_context *c);
// The SINR medium's tick: the frames of earlier ticks that are still on the air stay resident on the device (the window
// [air_head, air_tail) of d_air); the new ones are built from source indices (dev_src), or given as records in device memory
// or -- new_on_host -- in the host's pinned staging block, and join the window's tail.
int air_tick_device(rm_context *c, int64_t t_begin_us, const int32_t *dev_src, const rm_tx_record *dev_new, int32_t n, int64_t start_us,
                    int64_t air_us, int64_t latest_end_us, bool new_on_host);
int air_window_expire(rm_context *c, int64_t t_begin_us);
int air_window_reserve(rm_context *c, size_t n_more);
int result_device(rm_context *c, TickSlot &ts, rm_device_result *out);
int result_count(rm_context *c, TickSlot &ts, uint32_t *count, uint32_t *dropped);

// ---- rm_api_energy.cpp
// what the channel energy query refuses before anything is launched (the gated tick refuses the same)
int energy_check(rm_context *c, int64_t time_us, int32_t n, bool have_list);
// the query's index of the frames live at time_us, then the sum over `nodes` -- or, with `gated`, the gate of a gated tick over the
// candidates `nodes` (rm_energy.hip) -- on the context's stream; nodes / energy / flags are device-visible memory
int energy_launch(rm_context *c, int64_t time_us, const int32_t *nodes, int32_t n, int32_t channel, double cca_threshold, double *energy,
                  uint8_t *flags, int32_t *gated = nullptr);
// the host forms' pinned, host-mapped block with room for n nodes: energies, node list, flags
int energy_host_block(rm_context *c, int32_t n, double **h_energy, int32_t **h_nodes, uint8_t **h_flags);

// ---- rm_api_cca.cpp
// what a gated batch refuses before anything is launched: the arguments as such, then the ticks with the candidates each one senses
int cca_batch_check_lists(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *src,
                          const int32_t *n_src, const int64_t *start_us, const int64_t *air_us, const int64_t *cca_time_us);
int cca_batch_check_ticks(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int32_t *n_per, const int64_t *start_us,
                          const int64_t *air_us, const int64_t *cca_time_us);
// the gated batches' pinned, host-mapped block: tick descriptors, the device's words, `extra` bytes to upload from
int cca_desc_block(rm_context *c, size_t extra, rm::CcaTick **h_ticks, uint32_t **h_info, char **h_extra);
// the gate's buffers and device view for n_cand candidates (all of rm::CcaBatchDev but the pair list), descriptors written, gated_v[b] set
int cca_batch_dev(rm_context *c, size_t n_cand, int32_t n_ticks, const int32_t *const *src, const int32_t *n_per, const int64_t *start_us,
                  const int64_t *air_us, const int64_t *cca_time_us, size_t extra, rm::CcaBatchDev *out, bool *use_grid, rm::CcaTick **h_ticks_out,
                  const int32_t **gated_v, char **h_extra);

// ---- rm_api_errmodel.cpp: the frame error model (E10)
inline bool em_on(const rm_context *c) { return c->em.kind != RM_EM_NONE; }
rm::EmDev em_dev(const rm_context *c);

// ---- rm_api_stats.cpp: per-node traffic counters (E11)
inline bool stats_on(const rm_context *c) { return c->st.on; }
rm::StatsDev stats_dev(const rm_context *c);
// rm_nodes_upload: another node count resizes the table and zeroes it
int stats_nodes_changed(rm_context *c);

// ---- rm_api_listen.cpp: receiver listening schedules (E13)
inline bool listen_on(const rm_context *c) { return c->ls.on; }
rm::ListenDev listen_dev(const rm_context *c);
// rm_nodes_upload: another node count clears the feature
int listen_nodes_changed(rm_context *c);

// ---- rm_api_linkstats.cpp: watched-link statistics (E14)
inline bool linkstats_on(const rm_context *c) { return c->lk.K > 0; }
rm::LinkStatsDev linkstats_dev(const rm_context *c);
// rm_nodes_upload: another node count switches the feature off
int linkstats_nodes_changed(rm_context *c);
// rm_destroy: the tables and the host block
void linkstats_release(rm_context *c);
// what every call that reads or sets the tables refuses while the feature is off
int linkstats_have(const rm_context *c);
// the host's copy of the peer rows, read back from the device if rm_linkstats_watch_device has written the table since
int linkstats_host_fresh(rm_context *c);

// ---- rm_api_neighbors.cpp: the neighbour query (E16)
// rm_destroy
void neighbors_release(rm_context *c);

// ---- rm_api_hops.cpp: the hop query (E17)
// rm_destroy
void hops_release(rm_context *c);

// ---- rm_api_routes.cpp: the route query (E18)
// rm_destroy
void routes_release(rm_context *c);

// ---- rm_api_etx.cpp: the measured-route query (E21)
// rm_destroy
void etx_release(rm_context *c);

// ---- rm_api_traffic.cpp: traffic schedules (E15)
// rm_nodes_upload: another node count clears the feature
int traffic_nodes_changed(rm_context *c);
// rm_destroy
void traffic_release(rm_context *c);

// ---- rm_api_passes.cpp: the passes over a finished result (E10, E13, E11, E14 -- in this order; DESIGN.md, end of section 4.14)
// what an evaluating call refuses while a pass is on, before anything is launched: the gathered / rm_dist_* / rm_group_* forms
// (gathered), else a context with a receiver partition.  with_em: the frame error model's refusal is among them (the lone-tick
// entry points leave it to air_tick_device).  The members' form asks every member about one pass before the next pass
int passes_check(const rm_context *c, bool gathered, bool with_em);
int passes_check(const rm_context *const *members, size_t n, bool gathered, bool with_em);
// a pass that needs every tick as a slot's result with its compact arrays is on: the counters, the schedules, the watched links
bool passes_counting(const rm_context *c);
inline bool passes_any(const rm_context *c) { return passes_counting(c) || (em_on(c) && is_sinr(c)); }
// the passes behind a lone tick's launch sequence, dense form or not, over the slot's compact arrays (sinr: the tick is one of the
// SINR medium's, which alone runs E10)
int passes_tick(rm_context *c, TickSlot &ts, rm_context::Sample *smp, bool sinr);
// the passes over the n slots of a batch, one launch each, on the context's stream; the three behind E10's are sampled under
// counters_stage (E10's under RM_STAGE_SINR)
int passes_batch(rm_context *c, int n, const rm::TickDev *dev_ticks, rm_context::Sample *smp, int counters_stage);
// rm_nodes_upload: another node count -- the counters resize and zero, the schedules (E13, E15) clear, the watched links switch off
int passes_nodes_changed(rm_context *c);
// rm_destroy: the tables and host blocks of E11, E13, E14, E15 and E16
void passes_release(rm_context *c);

// ---- what the list calls of E11 .. E16 share
// a call that takes a node list or, without one, the whole table in node order
inline int check_node_list(const int32_t *nodes, int32_t n, int32_t n_nodes)
{
    if (!nodes && n != n_nodes) return fail(RM_ERR_INVALID, "without a list n has to be the node count");
    if (nodes)
        for (int32_t k = 0; k < n; ++k)
            if (nodes[k] < 0 || nodes[k] >= n_nodes) return fail(RM_ERR_INVALID, "node index out of range");
    return RM_OK;
}
// The tables of these calls are rows of `words` 64-bit words per node index (n_rows of them), and a list call moves rows through
// the table's PinnedBlock with the kernels of rm_rows.hip.
//
// A read of n rows into `out`, and of the totals where the table has them (dev_totals) and the caller asks (totals).  Without a
// list (the whole table in node order) or with n == 0 (the totals alone): copies on the stream, one synchronisation.  With a
// list: the list staged in the block, one gather launch, one synchronisation, then the copy out of the block
inline int rows_read(rm_context *c, PinnedBlock &h, const void *table, int words, int32_t n_rows, const int32_t *nodes, int32_t n, void *out,
                     const rm_stats_totals *dev_totals, rm_stats_totals *totals)
{
    const size_t row_bytes = size_t(words) * 8;
    if (!dev_totals) totals = nullptr;
    if (!nodes || n == 0) {
        if (n > 0) RM_HIP(hipMemcpyAsync(out, table, size_t(n) * row_bytes, hipMemcpyDeviceToHost, c->stream));
        if (totals) RM_HIP(hipMemcpyAsync(totals, dev_totals, sizeof(rm_stats_totals), hipMemcpyDeviceToHost, c->stream));
        RM_HIP(hipStreamSynchronize(c->stream));
        return RM_OK;
    }
    RM_TRY(h.ensure(c->stream, size_t(n), row_bytes));
    std::memcpy(h.nodes(), nodes, size_t(n) * 4);
    RM_HIP(rm::launch_rows_gather(c->stream, static_cast<const int64_t *>(table), words, n_rows, h.nodes(), n, reinterpret_cast<int64_t *>(h.rows()),
                                  dev_totals, totals ? h.totals() : nullptr));
    RM_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(out, h.rows(), size_t(n) * row_bytes);
    if (totals) *totals = *h.totals();
    return RM_OK;
}
// by list entry, the last entry that names the same node: entry k of a list update is staged from record rows_final(..)[k], so the
// last entry of a node wins (the list is validated: every node is below n_rows).  Lives in the block until its next list update
inline const int32_t *rows_final(PinnedBlock &h, const int32_t *nodes, int32_t n, int32_t n_rows)
{
    std::vector<int32_t> &v = h.last; // [n_rows] by node, then [n] by entry; only the nodes this list names are written and read
    v.resize(size_t(n_rows) + size_t(n));
    for (int32_t k = 0; k < n; ++k) v[size_t(nodes[k])] = k;
    for (int32_t k = 0; k < n; ++k) v[size_t(n_rows) + size_t(k)] = v[size_t(nodes[k])];
    return v.data() + n_rows;
}
// An update of the rows of a VALIDATED list: entry k staged in the block with row rec_row[k] of `recs` -- its node's FINAL record
// (rows_final over the caller's records, or the list itself over a host copy the list has been applied to), so duplicates write
// equal values -- then the list, and one scatter launch that is not waited for.  (The row is the record's type, so that staging
// a row is a copy of known size: with the size a run-time value, a list update of 100 000 schedules took a third longer)
template <typename Rec>
int rows_write(rm_context *c, PinnedBlock &h, Rec *table, int32_t n_rows, const int32_t *nodes, int32_t n, const Rec *recs, const int32_t *rec_row)
{
    static_assert(sizeof(Rec) % 8 == 0, "a row is whole 64-bit words");
    if (n < 1) return RM_OK;
    RM_TRY(h.ensure(c->stream, size_t(n), sizeof(Rec)));
    Rec *rows = reinterpret_cast<Rec *>(h.rows());
    for (int32_t k = 0; k < n; ++k) rows[k] = recs[rec_row[k]];
    std::memcpy(h.nodes(), nodes, size_t(n) * 4);
    RM_HIP(rm::launch_rows_scatter(c->stream, reinterpret_cast<int64_t *>(table), int(sizeof(Rec) / 8), n_rows, h.nodes(), n,
                                   reinterpret_cast<const int64_t *>(rows)));
    return RM_OK;
}
// a context made under RM_GRAPH=1 takes none of the extensions; `why` is the clause that names what is refused
inline int graphs_refuse(const rm_context *c, const char *why)
{
    if (!c->use_graphs) return RM_OK;
    return fail(RM_ERR_STATE, std::string("this context replays its ticks from captured graphs (RM_GRAPH=1): ") + why);
}

// ---- rm_api_unicast.cpp: the unicast outcome query (E12)
// an evaluating call has left its results in `slots` result slots (gathered: a gathered / rm_dist_* / rm_group_* form)
inline void uc_ran(rm_context *c, int slots, bool gathered)
{
    c->uc.slots = slots;
    c->uc.gathered = gathered;
}
// what every form refuses with RM_ERR_STATE: nothing launched, nothing changed
int uc_check_state(rm_context *c);
// the slot's compact arrays (written now if the tick left them for later), described for the kernel
int uc_describe(rm_context *c, TickSlot &ts, rm::UcSlot *d);
// the descriptors of all slots of the last call for the kernel (rm_api_unicast.cpp says how they travel)
int uc_slots(rm_context *c, bool all, const uint32_t *prefix, int n_prefix, rm::UcSlot *lone, const rm::UcSlot **dev_slots, const uint32_t **dev_prefix);

// ---- rm_api_fwd.cpp: forwarding queues (E19)
// rm_nodes_upload: another node count switches the feature off
int fwd_nodes_changed(rm_context *c);
// rm_destroy
void fwd_release(rm_context *c);

// ---- rm_api_flood.cpp: dissemination floods (E20)
// rm_nodes_upload: another node count switches the feature off
int flood_nodes_changed(rm_context *c);
// rm_destroy
void flood_release(rm_context *c);

// ---- rm_api_nbtable.cpp: neighbour tables (E22)
// the watched-link statistics go off (K = 0, another K, another node count; the stream has been waited for) and rm_destroy
void nbtable_release(rm_context *c);

// ---- rm_api_linkest.cpp: link estimator (E23)
// rm_nodes_upload: another node count switches the feature off
int linkest_nodes_changed(rm_context *c);
// rm_destroy
void linkest_release(rm_context *c);

// ---- rm_api_comm.cpp
int comm_all_gather(rm_context *c, const void *mine, void *all, size_t bytes);
int comm_finish_draws(rm_context *c);
int group_comm_init(rm_context *const *members, int n, void **comms_out);
int group_all_gather(rm_context *const *members, int n, const void *const *mine, void *const *all, size_t bytes);

// ---- rm_api_batch.cpp
TickSlot *slot_of(rm_context *c, int32_t slot);
// the launch sequence of n prepared ticks; m_override: the model the sweep runs with (a batch of overlapping SINR ticks
// sweeps with the medium without SINR), after_sweep: issued behind the last sweep stage, inside the sampled sequence
int launch_batch(rm_context *c, TickSlot *const *slots, const TickPlan *plans, int n, const rm::ModelDev *m_override = nullptr,
                 int (*after_sweep)(rm_context *, void *) = nullptr, void *after_arg = nullptr, const rm::RankFramesArgs *rank_frames = nullptr);
// a rank's frame list for tick `t` of a batch of gathered source indices (plan and slot prepared; n_pub gathered slots)
void nbr_cache_detach(rm_context *c);  // rm_destroy, behind its stream synchronize: leave the pool of heard lists; the last context frees it
void nbr_cache_report(rm_context *c); // RM_HOST_TIMING=1: what the source candidate cache served, in which form, and what was swept (stderr)
bool rank_frames_wanted(rm_context *c);
int plan_rank_frames(rm_context *c, TickSlot &ts, rm::TickDev &t, int n_pub);
// ---- rm_api_airbatch.cpp
bool overlap_wanted(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int32_t *n_per, const int64_t *start_us,
                    const int64_t *air_us);
int batch_run_overlap(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *dev_src,
                      const int32_t *n_per, const int64_t *start_us, const int64_t *air_us, const rm_tx_record *gathered, int gather_world,
                      int gather_slots, const int32_t *gathered_idx, int gather_block = 0, int digest_off = -1);
// gathered / gathered_idx: the ticks' frames where an all-gather of per-rank blocks left them, [rank][tick][slot] -- as records, or
// as source indices (then start_us / air_us give the ticks' time spans and every record is built from the node table)
int batch_run(rm_context *c, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us, const int32_t *const *dev_src,
              const rm_tx_record *const *dev_new, const int32_t *n_per, const int64_t *start_us, const int64_t *air_us,
              const rm_tx_record *gathered = nullptr, int gather_world = 0, int gather_slots = 0, const int32_t *gathered_idx = nullptr,
              int gather_block = 0, int digest_off = -1);
// (gather_block: elements from one rank's block of the gathered buffer to the next, 0 = n_ticks * gather_slots; digest_off: where
// in a rank's block of source indices its node-table digest lies -- two words, rm_table_digest -- or -1)

// ---- the relay features' scaffold (E19 rm_api_fwd.cpp, E20 rm_api_flood.cpp): rm_context::Relay, the feature's own words passed in
// (free_own releases the buffers the feature keeps beside the base's; off_msg is what a call says while the feature is off)
inline void relay_release(rm_context *c, rm_context::Relay &r, void (*free_own)(rm_context *))
{
    r.on = false;
    r.n = -1;
    free_own(c);
    r.claim.release(); r.unit_count.release(); r.stage.release();
    r.h.release();
}
// off: the tables released (a launch in flight still reads them; pointers handed out end here)
inline int relay_off(rm_context *c, rm_context::Relay &r, void (*free_own)(rm_context *))
{
    if (r.n >= 0 && c->stream) RM_HIP(hipStreamSynchronize(c->stream));
    relay_release(c, r, free_own);
    return RM_OK;
}
inline int relay_nodes_changed(rm_context *c, rm_context::Relay &r, void (*free_own)(rm_context *))
{
    if (r.n < 0 || r.n == c->n) return RM_OK;
    return relay_off(c, r, free_own);
}
inline int relay_have(const rm_context::Relay &r, const char *off_msg) { return r.on ? RM_OK : fail(RM_ERR_STATE, off_msg); }
// room for n entries of the running call in a block the stream's earlier calls may still use: a call that grows it waits for the
// stream first.  (Enable sizes the per-entry records for n_nodes entries: only a list longer than the node table grows them)
template <typename T> int relay_room(rm_context *c, DevBuf<T> &b, size_t n)
{
    n = std::max<size_t>(n, 1);
    if (b.n >= n) return RM_OK;
    RM_HIP(hipStreamSynchronize(c->stream));
    RM_HIP(b.ensure(n));
    return RM_OK;
}
inline int relay_check_host_list(const rm_context::Relay &r, const int32_t *list, int32_t n, const char *what)
{
    for (int32_t k = 0; k < n; ++k)
        if (list[k] >= r.n) return fail(RM_ERR_INVALID, std::string("an entry of the host ") + what + " list is not below the node count");
    return RM_OK;
}
// a host form's list in device memory (r.stage.p), there when this returns
inline int relay_stage_list(rm_context *c, rm_context::Relay &r, const int32_t *list, int32_t n)
{
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_room(c, r.stage, size_t(n)));
    if (n < 1) return RM_OK;
    RM_HIP(hipMemcpyAsync(r.stage.p, list, size_t(n) * 4, hipMemcpyHostToDevice, c->stream));
    RM_HIP(hipStreamSynchronize(c->stream));
    return RM_OK;
}
// the source list, device form: launch(units, chunk, dev_src, dev_count) is the feature's three launches
template <typename Launch>
int relay_sources_device(rm_context *c, rm_context::Relay &r, const char *off_msg, int64_t time_us, int32_t cap, int32_t *dev_src, int32_t *dev_count,
                         Launch launch)
{
    if (!dev_src || !dev_count || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    if (cap < 1) return fail(RM_ERR_INVALID, "cap < 1");
    RM_TRY(relay_have(r, off_msg));
    RM_HIP(hipSetDevice(c->device));
    int units = 0, chunk = 0;
    rm::traffic_geometry(r.n, &units, &chunk);
    if (r.unit_count.n < size_t(units)) return fail(RM_ERR_STATE, "internal: the units' counts were sized for another node count");
    CallProbe probe(c);
    RM_HIP(launch(units, chunk, dev_src, dev_count));
    return RM_OK;
}
// ... and the host form: the list and its count through the staging block, waited for
template <typename Launch>
int relay_sources(rm_context *c, rm_context::Relay &r, const char *off_msg, int64_t time_us, int32_t cap, int32_t *src, int32_t *count, Launch launch)
{
    if (!src || !count || time_us < 0) return fail(RM_ERR_INVALID, "bad arguments");
    if (cap < 1) return fail(RM_ERR_INVALID, "cap < 1");
    RM_TRY(relay_have(r, off_msg));
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(relay_room(c, r.stage, size_t(cap) + 1));
    int32_t *d = r.stage.p;
    RM_TRY(relay_sources_device(c, r, off_msg, time_us, cap, d, d + cap, launch));
    RM_HIP(hipMemcpyAsync(src, d, size_t(cap) * 4, hipMemcpyDeviceToHost, c->stream));
    RM_HIP(hipMemcpyAsync(count, d + cap, 4, hipMemcpyDeviceToHost, c->stream));
    RM_HIP(hipStreamSynchronize(c->stream));
    return RM_OK;
}
// what both advance forms check, in this order, before anything else happens
inline int relay_check_advance(rm_context *c, const rm_context::Relay &r, const char *off_msg, int32_t slot, int32_t n_cand)
{
    if (n_cand < 0) return fail(RM_ERR_INVALID, "bad arguments");
    RM_TRY(relay_have(r, off_msg));
    RM_TRY(uc_check_state(c));
    if (slot < 0 || slot >= c->uc.slots) return fail(RM_ERR_INVALID, "slot outside the slots of the last evaluating call");
    return RM_OK;
}
// the device form's way to its launches: the checks, the finished slot described for the kernels, P packet numbers to look at
inline int relay_advance_begin(rm_context *c, const rm_context::Relay &r, const char *off_msg, int32_t slot, const int32_t *dev_cand, int32_t n_cand,
                               rm::UcSlot *d, int32_t *P)
{
    RM_TRY(relay_check_advance(c, r, off_msg, slot, n_cand));
    RM_HIP(hipSetDevice(c->device));
    RM_TRY(uc_describe(c, *slot_of(c, slot), d));
    *P = dev_cand ? std::min(n_cand, d->n_new) : d->n_new;
    return RM_OK;
}

} // namespace rmh
