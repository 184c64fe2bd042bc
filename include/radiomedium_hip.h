/*
 * radiomedium_hip.h -- C ABI of libradiomedium_hip.so, the MI355X (gfx950) engine for
 * radio-sim's per-packet propagation / delivery-verdict pass.
 *
 * This is the drop-in boundary for the reference's RadioMedium plug-in contract
 * (reference paths relative to /root/reference/radio-medium/java/se/sics/emul8/radiomedium/):
 *
 *     public interface RadioMedium {            RadioMedium.java:35-45
 *         String getName();                     -> rm_get_name
 *         void   setSimulator(Simulator sim);   -> rm_create / rm_nodes_upload / rm_seed / rm_set_time
 *         void   transmit(RadioPacket packet);  -> rm_transmit   (or rm_enqueue_tx + rm_tick_flush)
 *         double getBaseRSSI(Node node);        -> rm_get_base_rssi
 *     }
 *
 * Plain C types only (pointers + sizes); no exceptions cross it; every function returns an
 * int status (RM_OK or a negative RM_ERR_*) unless stated, and rm_last_error() gives the
 * thread-local message of the last failure.  A context is NOT re-entrant: the caller
 * serialises calls per context (the reference enters transmit() from per-socket reader
 * threads, net/JSONClientConnection.java:118-131; the Java shim in INTEGRATION.md holds
 * one lock).  There is no CPU fallback: without a usable HIP device rm_create fails with
 * RM_ERR_NO_DEVICE.
 *
 * Node indices are positions in Simulator.getNodes() (registration order,
 * Simulator.java:245,274) -- the order the reference's loop visits receivers in, and the
 * order heard links are returned in.
 */
#ifndef RADIOMEDIUM_HIP_H
#define RADIOMEDIUM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5: rm_host_result.rssi is NULL for the reference's four media and pkt_rssi carries one value per packet;
 *    a partitioned context that is handed all ranks' source indices keeps, per tick, only the frames that can matter to
 *    its receivers (results unchanged: packets keep their numbers); the ranks' node-table digests ride in the all-gather of
 *    rm_dist_batch_run_sources_device (rm_table_digest, rm_batch_run_gathered_blocks_device, RM_GATHER_TRAILER): a rank
 *    whose copy of the node table differs makes the batch RM_ERR_STATE on every rank.
 * 4: rm_profile_enable times every kernel by its own dispatch (rm_profile_kernels; RM_STAGE_EMPTY is always 0);
 *    rm_batch_run_sources_device / rm_batch_run_gathered_sources_device / rm_dist_batch_run_sources_device take ticks of
 *    the SINR medium whose frames outlive their tick (rm_air_batch_stats); rm_node_info_changed.
 * 3: rm_host_result.pkt is NULL (a link's packet follows from pkt_offset: the column no longer crosses PCIe) and so is
 *    rm_delivery_view.packet (the packet numbers come once per run of deliveries: n_runs, run_*); rm_air_scan_ticks,
 *    rm_batch_run_gathered_sources_device.
 * 2: rm_delivery_view.oldest_packet; rm_host_result.sinr / rm_device_result.sinr are NULL without the SINR extension;
 *    rm_group_*, rm_events_*, rm_node_info, rm_tick_run_records_device, rm_set_partition_spatial and the draw-node
 *    exchange were added; rm_tick_run_device refuses the SINR medium (rm_tick_run_records_device takes it).  A host
 *    built against another version must not load this library: compare rm_abi_version() with RM_ABI_VERSION. */
#define RM_ABI_VERSION 5

#define RM_OK 0
#define RM_ERR_INVALID (-1)   /* bad argument */
#define RM_ERR_NO_DEVICE (-2) /* no usable HIP device / library built without one */
#define RM_ERR_HIP (-3)       /* a HIP runtime call failed */
#define RM_ERR_CAPACITY (-4)  /* caller buffer or link capacity too small (count is still returned) */
#define RM_ERR_STATE (-5)     /* call sequence / configuration not valid for this call */

typedef struct rm_context rm_context;

/* which RadioMedium implementation the context behaves as */
enum rm_model_kind {
    RM_MODEL_NULL = 0,       /* NullRadioMedium.java:47-77 */
    RM_MODEL_UDGM = 1,       /* UDGMRadioMedium.java:63-117 */
    RM_MODEL_UDGM_CONST = 2, /* UDGMConstantLossRadioMedium.java:16-36 */
    RM_MODEL_N2N = 3,        /* N2NRadioMedium.java:24-73 */
    RM_MODEL_LOGDIST = 4     /* build-defined extension, DESIGN.md "Extension spec" */
};

/* events/ReceptionEvent.java:12-16: unheard links are never reported */
enum rm_verdict { RM_UNHEARD = 0, RM_INTERFERED = 1, RM_DELIVERED = 2 };

#define RM_LD_SINR 1 /* logdist: co-channel SINR capture + half duplex over the on-air list */

typedef struct rm_model_params {
    int32_t kind;  /* enum rm_model_kind */
    int32_t flags; /* RM_LD_* */
    /* UDGMRadioMedium.java:18-24 (setters :31-61) */
    double udgm_success_ratio_tx;   /* declared by the reference, never used (kept for parity) */
    double udgm_success_ratio_rx;
    double udgm_transmission_range;
    double udgm_interference_range; /* declared by the reference, never read */
    /* UDGMConstantLossRadioMedium.java:8 */
    double const_range;
    /* extension */
    double ld_pl0_db, ld_exponent, ld_d0;
    double ld_sigma_db, ld_clip;
    uint64_t ld_seed;
    double ld_sensitivity_dbm, ld_noise_dbm, ld_capture_db, ld_ifloor_dbm;
} rm_model_params;

/* One frame on the air: RadioPacket.java:40-52 plus the source state transmit() reads
 * (source position, Position.java; txProbability, Transciever.java:18).  This is also the
 * record the ranks all-gather each tick in the receiver-sharded multi-GPU mode. */
typedef struct rm_tx_record {
    double x, y, z;
    double txpower;
    double txprob;
    int64_t start_us;
    int64_t air_us;
    int32_t src;
    int32_t channel;
} rm_tx_record; /* 64 bytes */

/* device-resident result of the last evaluated tick (all pointers are device memory owned by
 * the context, valid until the next rm_tick_* / rm_transmit call) */
typedef struct rm_device_result {
    const uint32_t *count;      /* [1] heard links */
    const uint32_t *pkt_offset; /* [n_new+1] first link of each new packet */
    const int32_t *pkt;         /* [count] index into this tick's new packets */
    const int32_t *dst;         /* [count] receiver node index */
    const uint8_t *verdict;     /* [count] RM_INTERFERED / RM_DELIVERED */
    const double *rssi;         /* [count] */
    const double *sinr;         /* [count] with the SINR extension, else NULL (host copies deliver 0) */
    uint32_t capacity;
} rm_device_result;

/* ---- life cycle ---------------------------------------------------------------------- */
int rm_abi_version(void);
int rm_device_count(void);                              /* >=0, or RM_ERR_* */
int rm_create(int device_ordinal, rm_context **out);    /* Simulator.setRadioMedium(...) -> setSimulator */
void rm_destroy(rm_context *ctx);
const char *rm_last_error(void);
const char *rm_get_name(const rm_context *ctx);         /* RadioMedium.getName() */
int rm_set_stream(rm_context *ctx, void *hip_stream);   /* all work is enqueued on this stream */

/* ---- model ---------------------------------------------------------------------------- */
void rm_model_defaults(rm_model_params *p, int32_t kind); /* the reference's field defaults */
int rm_set_model(rm_context *ctx, const rm_model_params *p);
int rm_get_model(const rm_context *ctx, rm_model_params *out);
/* N2NRadioMedium(double[][] m): row-major m x m (net/SimulatorJSONHandler.java:183-206) */
int rm_set_n2n_matrix(rm_context *ctx, int32_t m, const double *row_major);
int rm_set_base_rssi(rm_context *ctx, double rssi);       /* AbstractRadioMedium.java:51-53 */
double rm_get_base_rssi(const rm_context *ctx, int32_t node); /* RadioMedium.getBaseRSSI */

/* ---- Simulator.getRandom(): one java.util.Random shared by all packets ------------------ */
int rm_seed(rm_context *ctx, int64_t seed);               /* new java.util.Random(seed) */
int rm_get_rng_state(rm_context *ctx, uint64_t *state48);
int rm_set_rng_state(rm_context *ctx, uint64_t state48);

/* ---- node state (Simulator.getNodes() snapshot; Node/Position/Transciever fields) -------- */
int rm_nodes_upload(rm_context *ctx, int32_t n,
                    const double *x, const double *y, const double *z,
                    const double *txpower, const int32_t *channel, const uint8_t *enabled,
                    const double *rxprob, const double *txprob,
                    const int32_t *int_id /* Node.getIdAsInteger(); NULL = index+1 */);
/* One changed node (node-config-set, SimulatorJSONHandler.java:105-143: position, rf-power,
 * wireless-channel, rx-loss, tx-loss, radio-state).  Written in place on the device by one small
 * launch, no synchronisation; the receiver table is sorted again only after enough receivers have
 * left the box their group of 64 had (results never depend on that order). */
int rm_node_update(rm_context *ctx, int32_t node, double x, double y, double z, double txpower,
                   int32_t channel, uint8_t enabled, double rxprob, double txprob);
/* New positions of `count` nodes in one call (Position.set, Position.java:44-52); z may be NULL
 * (z = 0, as Position.set(x, y) does).  The shim's "dirty list" flushed at the start of a tick. */
int rm_nodes_move(rm_context *ctx, int32_t count, const int32_t *nodes, const double *x, const double *y,
                  const double *z);
/* how often the receiver table has been (re)built and spatially sorted so far (observability) */
int64_t rm_receiver_table_builds(const rm_context *ctx);
int rm_node_count(const rm_context *ctx);
/* receiver range owned by this context (multi-GPU range partitioning); default = all */
int rm_set_partition(rm_context *ctx, int32_t first, int32_t count);
/* Receivers partitioned by REGION instead of by index range: this context owns part `part` of the `n_parts` regions the
 * k-d split of ALL node positions yields (groups of 64 nodes in proportion; ties by node index, so every rank computes the
 * same cut from the same table for itself).  A rank's receivers then lie together, its filter drops the frames far from
 * its region, and a packet's heard links -- still ascending in node index inside every rank -- are merged by node index
 * across the ranks.  The members are fixed until the next rm_nodes_upload / partition call: a node that moves stays with
 * its rank.  n_parts == 1: no partition.  rm_partition_of_nodes labels every node with its part (which rank owns a source,
 * for the all-gather of Tx records); rm_partition_nodes lists this context's receivers in ascending order. */
int rm_set_partition_spatial(rm_context *ctx, int32_t part, int32_t n_parts);
int rm_partition_of_nodes(rm_context *ctx, int32_t n_parts, int32_t *part_of /* [n] */);
int rm_partition_nodes(rm_context *ctx, int32_t *nodes, int32_t cap, int32_t *count);
/* the same cut from positions alone (host only, no context, no device): what rm_partition_of_nodes answers for a table
 * with these positions (z may be NULL: 0) */
int rm_region_split(int32_t n, const double *x, const double *y, const double *z, int32_t n_parts, int32_t *part_of /* [n] */);
int rm_set_link_capacity(rm_context *ctx, uint32_t max_links);

/* ---- time ------------------------------------------------------------------------------ */
int rm_set_time(rm_context *ctx, int64_t current_time_us);          /* Simulator.getTime() */
int64_t rm_air_time_us(int64_t hex_length);                         /* RadioPacket.java:67-75 */
/* Simulator.java:321-335: event times of a packet given the simulator's current time */
void rm_event_times(int64_t start_us, int64_t air_us, int64_t current_time_us,
                    int64_t *t_start, int64_t *t_end);

/* ---- transmit(): one packet, reference semantics ------------------------------------------
 * txpower / channel: optional overrides ("rf-power", "wireless-channel",
 * net/SimulatorJSONHandler.java:83-90); NULL = the source radio's values.
 * Heard receivers are returned in node order.  *count gets the number of heard links even
 * when it exceeds cap (then RM_ERR_CAPACITY).  interference (may be NULL) gets the packet
 * level Tx-failure flag (UDGMRadioMedium.java:88-92). */
int rm_transmit(rm_context *ctx, int32_t src, int64_t start_us, int64_t hex_length,
                const double *txpower, const int32_t *channel,
                int32_t *dst, uint8_t *verdict, double *rssi, double *sinr, uint32_t cap,
                uint32_t *count, uint8_t *interference);

/* ---- batched: all frames of one simulated tick in one pass -------------------------------- */
int rm_tick_begin(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us);
int rm_enqueue_tx(rm_context *ctx, int32_t src, int64_t start_us, int64_t air_us,
                  const double *txpower, const int32_t *channel);
/* records built by the caller: a record's txprob decides the packet's Tx draw (UDGMRadioMedium.java:87-92), also
 * where it differs from the node table */
int rm_enqueue_tx_records(rm_context *ctx, const rm_tx_record *recs, int32_t n);
/* evaluates the tick and copies the heard links (packet-major, receiver ascending) out */
int rm_tick_flush(rm_context *ctx, int32_t *pkt, int32_t *dst, uint8_t *verdict,
                  double *rssi, double *sinr, uint32_t cap, uint32_t *count,
                  uint8_t *pkt_interference /* [n_new] or NULL */,
                  uint32_t *pkt_offset /* [n_new+1] or NULL */);

/* The same without the copy: the engine's last kernel writes the tick's result into pinned,
 * host-mapped memory the context owns, and the caller reads it in place (a JNI shim wraps the
 * arrays in direct ByteBuffers).  The pointers stay valid until the next call that evaluates
 * anything on this context.  `count` records are there; an error is reported as by rm_tick_flush. */
typedef struct rm_host_result {
    uint32_t count;                  /* heard links */
    uint32_t n_packets;              /* frames of this tick */
    const uint32_t *pkt_offset;      /* [n_packets + 1] first link of every packet */
    const uint8_t *pkt_interference; /* [n_packets] Tx-failure flag (UDGMRadioMedium.java:88-92) */
    const int32_t *pkt;              /* NULL since ABI version 3: link i belongs to the packet q with pkt_offset[q] <= i < pkt_offset[q + 1]
                                      * (4 of a record's 17 bytes that need not cross PCIe; rm_tick_flush still fills its caller's array) */
    const int32_t *dst;              /* [count] receiver node index (ascending per packet) */
    const uint8_t *verdict;          /* [count] RM_INTERFERED / RM_DELIVERED */
    const double *rssi;              /* [count] -- or NULL (ABI version 5) for the reference's four media: a heard link's rssi is its
                                      * packet's transmit power there (UDGMRadioMedium.java:95, NullRadioMedium.java:57,
                                      * N2NRadioMedium.java:51, UDGMConstantLossRadioMedium.java:22), and it crosses PCIe once per packet: */
    const double *sinr;              /* [count] with the SINR extension, else NULL (as rm_device_result.sinr) */
    const double *pkt_rssi;          /* [n_packets] when rssi is NULL: link i of packet q has rssi pkt_rssi[q] (5 bytes per link
                                      * instead of 13); NULL when rssi is not (rm_tick_flush still fills its caller's array) */
} rm_host_result;
int rm_tick_flush_view(rm_context *ctx, rm_host_result *out);

/* A medium in which a frame is heard by a large share of all nodes -- the reference's default NullRadioMedium (every same-channel
 * node: NullRadioMedium.java:62-73), a unit disc over a small field (not the N2N matrix: its ticks take the general path) -- is
 * evaluated in node order, and
 * what its tick leaves IS its result: per (packet, chunk of 1024 consecutive nodes) cell sixteen 64-bit lane masks -- bit l
 * of mask k set: node rx_first + 1024 * chunk + 64 * k + l heard the packet -- and the cell's count.  A heard link's rssi is
 * its packet's transmit power, its verdict its packet's (pkt_interference): nothing else distinguishes links of such a medium,
 * so the 17-byte records (68 MB for 4 M links) are written only when rm_result_device / rm_result_copy / a host view asks.
 * The tick itself ends with the masks and the cells' counts (one launch); the packets' offsets and the total are laid out on the
 * context's stream when this call (or rm_result_count) first asks for them.
 * All pointers are device memory, valid until the next evaluating call; RM_ERR_STATE when the last tick took another form. */
typedef struct rm_dense_result {
    const unsigned long long *cell_mask; /* [n_packets][chunks][16] */
    const uint32_t *cell_count;          /* [n_packets][chunks] */
    const uint32_t *count;               /* [1] heard links of the tick */
    const uint32_t *pkt_offset;          /* [n_packets + 1] */
    const uint8_t *pkt_interference;     /* [n_packets] */
    int32_t n_packets, chunks, rx_first;
} rm_dense_result;
int rm_result_dense(rm_context *ctx, rm_dense_result *out);

/* evaluate the enqueued tick without copying anything out (then rm_result_copy / rm_result_device) */
int rm_tick_run(rm_context *ctx);

/* ---- receiver partitions with probabilistic links --------------------------------------------
 * The shared java.util.Random is consumed in packet order, then node order = rank order, so a
 * rank needs every rank's per-packet draw counts before it can place its own draws.  After
 * rm_tick_run / rm_tick_run_device on a partitioned context whose links may draw,
 * rm_draws_pending() is 1: all-gather rm_draw_counts_device (uint32[n_new] per rank, rank-major)
 * and call rm_tick_finish_draws; only then are verdicts, Tx-failure flags and the generator
 * state final (identical on all ranks). */
int rm_draws_pending(const rm_context *ctx);
int rm_draw_counts_device(rm_context *ctx, const uint32_t **dev_counts, int32_t *n_new);
int rm_draw_counts_to(rm_context *ctx, uint32_t *dev_out); /* async copy into a caller's device buffer */
int rm_tick_finish_draws(rm_context *ctx, const uint32_t *all_counts /* [world][n_new] */, int32_t world,
                         int32_t rank, int on_device);
/* Spatial partitions (rm_set_partition_spatial): the ranks' node sets interleave in node order, so the counts are not
 * enough -- every rank also publishes the node index of each of its links that will draw, packet-major, ascending inside
 * a packet (rm_draw_nodes_device: sum of its counts entries), the lists are all-gathered into rows of `stride` entries
 * per rank, and a link's place among its packet's draws is the number of listed nodes below it over all ranks. */
int rm_draw_nodes_device(rm_context *ctx, const int32_t **dev_nodes);
int rm_tick_finish_draws_nodes(rm_context *ctx, const uint32_t *all_counts /* [world][n_new] */,
                               const int32_t *all_nodes /* [world][stride] */, uint32_t stride, int32_t world, int on_device);

/* ---- device-resident path (bench, multi-GPU): no host copies ------------------------------ */
/* build tx records for sources `dev_src[0..n)` from the resident node state */
int rm_pack_tx_device(rm_context *ctx, const int32_t *dev_src, int32_t n, int64_t start_us,
                      int64_t air_us, rm_tx_record *dev_out);
/* the same on another stream (packing + all-gather of tick t+1 can overlap the sweep of tick t) */
int rm_pack_tx_device_on(rm_context *ctx, void *hip_stream, const int32_t *dev_src, int32_t n,
                         int64_t start_us, int64_t air_us, rm_tx_record *dev_out);
/* the same for n_ticks ticks in one launch: dev_src / dev_out hold n_ticks rows of n entries, row b
 * starts at start_us[b] (host array) -- feeds one RCCL all-gather per batch of ticks */
int rm_pack_tx_batch_device_on(rm_context *ctx, void *hip_stream, const int32_t *dev_src, int32_t n_ticks, int32_t n,
                               const int64_t *start_us, int64_t air_us, rm_tx_record *dev_out);
/* evaluate one tick whose new frames are `dev_new[0..n_new)` (device memory, canonical order).  Records in device
 * memory are not inspected by the host: their txprob has to be the source node's (as rm_pack_tx_device builds
 * them) -- whether a java.util.Random draw can happen is decided from the node table and the model. */
int rm_tick_run_device(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us,
                       const rm_tx_record *dev_new, int32_t n_new);
/* the same with the new frames given as source node indices (device int32[n], -1 = padding): the
 * Tx records are built from the resident node state inside the sweep -- RadioPacket(node, time,
 * data) copies txpower / channel from its source, RadioPacket.java:46-52 -- one call per tick */
int rm_tick_run_sources_device(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us,
                               const int32_t *dev_src, int32_t n, int64_t start_us, int64_t air_us);
/* as rm_tick_run_device for the SINR extension, whose frames stay on the air over several ticks (the gathered records
 * of a receiver-sharded tick): `latest_end_us` is an upper bound of start + air over the records
 * -- the host never reads them and has to know how long their entries can matter.  The engine keeps a copy of the
 * records while they are on the air.  Without the SINR extension this is rm_tick_run_device. */
int rm_tick_run_records_device(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us, const rm_tx_record *dev_new,
                               int32_t n_new, int64_t latest_end_us);
int rm_result_device(rm_context *ctx, rm_device_result *out);
int rm_result_count(rm_context *ctx, uint32_t *count, uint32_t *dropped); /* synchronises */
/* copy the last evaluated tick's heard links to host buffers (same layout as rm_tick_flush) */
int rm_result_copy(rm_context *ctx, int32_t *pkt, int32_t *dst, uint8_t *verdict, double *rssi,
                   double *sinr, uint32_t cap, uint32_t *count, uint8_t *pkt_interference,
                   uint32_t *pkt_offset);
int rm_sync(rm_context *ctx);

/* ---- several independent ticks per pass ---------------------------------------------------------
 * RadioMedium.transmit treats every packet on its own (UDGMRadioMedium.java:63-117 reads nothing
 * but the packet, the node table and the shared Random), so the frames of n_ticks consecutive
 * ticks can be swept together: one launch sequence for all of them instead of one per tick,
 * which is what fills an MI355X at the 100k-node sizes (a single tick is a few dependent
 * launches of a few microseconds each).  Tick b's results live in result slot b of the context
 * (slot 0 is also what rm_result_* read) until the next rm_batch_* / rm_tick_* call.  The
 * java.util.Random draws are consumed tick by tick in slot order, i.e. exactly as n_ticks
 * single rm_tick_run_sources_device calls would.
 * The RM_LD_SINR extension looks at every frame on the air.  With source indices (rm_batch_run_sources_device and the
 * gathered-sources forms) the frames' time spans are in the arguments, and both kinds of batch are taken:
 *  - self-contained ticks (no frame of an earlier call or of an earlier tick of the batch still on the air when a tick
 *    begins: air time <= tick length) keep per-tick interferer lists inside the sweep;
 *  - ticks whose frames OUTLIVE them (BASELINE configs[4]: 8128 us frames over 1000 us ticks), or that begin while frames
 *    of earlier calls are on the air: the heard links of all ticks come from the sweep of the medium without SINR, then
 *    every frame the batch can see -- the context's on-air window, then the batch's ticks -- is indexed once and the
 *    interference sums of all ticks are formed in bulk (rm_airbatch.hip).  A frame's verdicts are decided against the
 *    frames of its own and earlier ticks, exactly as n_ticks single calls would decide them; the batch's frames join the
 *    on-air window for the calls that follow.  The ticks have to be in time order and their links must not draw.
 * With records (rm_batch_run_device, rm_batch_run_gathered_device) the host cannot see the time spans: the ticks
 * [t_begin, t_end] must not overlap and every frame has to lie inside its tick -- verified on the device, a violation is
 * reported as RM_ERR_STATE when the tick's result is read.  Anything else of it, and partitioned contexts whose links draw,
 * are refused with RM_ERR_STATE -- run those one tick at a time. */
#define RM_MAX_BATCH 512
int rm_batch_run_sources_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us /* [n_ticks] */,
                                const int64_t *t_end_us, const int32_t *const *dev_src /* device int32[n_src[b]] each */,
                                const int32_t *n_src, const int64_t *start_us, const int64_t *air_us);
/* the same with the ticks' Tx records given (device memory, canonical order), as rm_tick_run_device */
int rm_batch_run_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                        const rm_tx_record *const *dev_new, const int32_t *n_new);
/* the same with the ticks' records where an all-gather of per-rank blocks left them: dev_gathered[rank][tick][slot]
 * (`world` ranks, each packed `slots` records per tick for all n_ticks ticks, src = -1 = padding); tick b's packets are
 * the world * slots records dev_gathered[(r * n_ticks + b) * slots + s], rank-major -- no transposition in between */
int rm_batch_run_gathered_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                 const rm_tx_record *dev_gathered, int32_t world, int32_t slots);
/* the same from the ticks' SOURCE INDICES where an all-gather of per-rank blocks left them: dev_src_all[rank][tick][slot]
 * (-1: padding; all frames of tick b start at start_us[b] and last air_us).  Every rank holds the whole node table, so
 * it builds the records of all ranks' frames itself: what has to cross the links between the GPUs is 4 bytes per frame
 * instead of a 64-byte record (rm_dist_batch_run_sources_device does exactly this around its ncclAllGather) */
int rm_batch_run_gathered_sources_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                         const int32_t *dev_src_all, int32_t world, int32_t slots, const int64_t *start_us,
                                         int64_t air_us);
/* the same with every rank's block as rm_dist_batch_run_sources_device's own all-gather leaves it: n_ticks * slots source
 * indices followed by RM_GATHER_TRAILER words, the first two of them the rank's rm_table_digest (low word, high word).
 * Every rank builds the other ranks' records from ITS copy of the node table (the reference has no change hook --
 * net/SimulatorJSONHandler.java:105-143 -- so a host may miss an update): a block whose digest differs from this
 * context's makes every tick of the batch read as RM_ERR_STATE. */
#define RM_GATHER_TRAILER 4
int rm_batch_run_gathered_blocks_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                        const int32_t *dev_blocks /* [world][n_ticks * slots + RM_GATHER_TRAILER] */, int32_t world,
                                        int32_t slots, const int64_t *start_us, int64_t air_us);
/* digest of the node table as this context holds it: a function of its content (node count and every node's fields),
 * whatever sequence of rm_nodes_upload / rm_node_update / rm_nodes_move calls produced it */
int rm_table_digest(const rm_context *ctx, uint64_t *digest);
/* ticks of the last batch a filter workgroup swept with one load of its 1024 receivers: the receiver table left HBM once per
 * that many ticks of the launch (what a roofline has to charge the launch for the table) */
int rm_batch_tile_reuse(const rm_context *ctx);
int rm_batch_result_device(rm_context *ctx, int32_t slot, rm_device_result *out);
int rm_batch_result_count(rm_context *ctx, int32_t slot, uint32_t *count, uint32_t *dropped); /* synchronises */
int rm_batch_result_copy(rm_context *ctx, int32_t slot, int32_t *pkt, int32_t *dst, uint8_t *verdict, double *rssi,
                         double *sinr, uint32_t cap, uint32_t *count, uint8_t *pkt_interference,
                         uint32_t *pkt_offset);
/* The results of slots 0 .. n_slots-1 in the context's pinned, host-mapped block: one packing
 * launch, one wait; out[b] points into the block (valid until the next evaluating call).
 * status (may be NULL) gets every slot's own RM_OK / RM_ERR_CAPACITY / RM_ERR_STATE; the return
 * value is the first of them that is not RM_OK. */
int rm_batch_result_view(rm_context *ctx, int32_t n_slots, rm_host_result *out, int32_t *status);

/* Kernel timing on the context's stream: on every `every_n`-th launch sequence (0 = off) every kernel launch carries its
 * own pair of HIP events (hipExtLaunchKernelGGL), which take the start and the end of THAT dispatch -- the interval a
 * rocprofv3 kernel trace reports for it, without the launch gap before it and without whatever other contexts have in
 * flight.  rm_profile_read returns the number of sampled sequences and the summed kernel milliseconds per stage,
 * rm_profile_kernels the same per kernel, under the name rocprofv3 prints (template arguments as the launch site spells them).
 * The launches of rm_events_process and rm_node_info are sequences of their own, sampled while the count of evaluated ticks is
 * a multiple of every_n (they do not move it on): k_ev_append_select tells a drain that took the last tick's append into its
 * first launch from one that found it done (k_ev_select; k_ev_append, where rm_node_info had to flush it). */
enum rm_profile_stage {
    RM_STAGE_FILTER = 0,  /* k_filter (or k_tick_prep + k_filter_wg): all (frame, receiver) pairs, conservative */
    RM_STAGE_EXACT = 1,   /* k_exact: the reference's fp64 arithmetic on the candidates */
    RM_STAGE_SELF = 2,    /* k_self_entries (SINR) */
    RM_STAGE_OFFSETS = 3, /* k_cell_off + k_slot_scan */
    RM_STAGE_SINR = 4,    /* k_sinr */
    RM_STAGE_SCATTER = 5, /* k_finalize */
    RM_STAGE_REORDER = 6, /* k_reorder */
    RM_STAGE_DRAWS = 7,   /* java.util.Random kernels */
    RM_STAGE_EMPTY = 8,   /* unused since ABI version 4 (was: the cost of an event bracket); always 0 */
    RM_PROFILE_STAGES = 9
};
int rm_profile_enable(rm_context *ctx, int every_n);
int rm_profile_read(rm_context *ctx, uint32_t *samples, double *stage_ms /* [RM_PROFILE_STAGES] */);
typedef struct rm_kernel_time {
    char name[96];      /* e.g. "k_filter_wg_batch<4, true>" */
    int32_t stage;      /* rm_profile_stage the launch belongs to */
    uint32_t launches;  /* sampled launches */
    double total_ms;    /* their summed duration */
} rm_kernel_time;
/* count gets the number of distinct kernels sampled since rm_profile_enable; at most cap entries are written */
int rm_profile_kernels(rm_context *ctx, rm_kernel_time *out, int32_t cap, int32_t *count);
/* number of Tx->Rx link evaluations resolved by the last tick ( T * (N_loc) minus self links ) */
int64_t rm_last_link_evaluations(const rm_context *ctx);
/* observability (synchronises): the candidate links the sweep's conservative filter handed to the exact stage for the
 * tick of result slot `slot` (0 on the one-launch tick path, which keeps no candidate list) and its heard links.  A frame
 * that a draw-free batch served from its source's cached records (the heard form) was neither swept nor
 * evaluated: the candidate count holds the SWEPT frames' candidates only, the heard count every frame's links */
int rm_slot_stats(rm_context *ctx, int32_t slot, uint64_t *candidates, uint64_t *heard);
/* the SINR extension's on-air lists (build-defined, DESIGN.md "Extension spec" E4): how many ticks added only their new
 * frames to the per-receiver interferer lists kept on the device, and how many rebuilt the lists from every frame on the
 * air (first tick, after a node / model / partition / capacity change, after a dropped tick, when t_begin went back) */
int rm_air_list_stats(const rm_context *ctx, uint64_t *incremental_ticks, uint64_t *rebuilt_ticks);
/* ... and how many ticks needed no lists at all: a tick of at most 4096 new frames over a spatially sorted table finds the
 * interferers of its heard links among the frames on the air themselves (rm_airscan.hip; RM_SINR_SCAN=0 keeps the lists) */
int rm_air_scan_ticks(const rm_context *ctx, uint64_t *scan_ticks);
/* ... and the batches of ticks whose frames outlive their tick (rm_batch_run_sources_device and the gathered-sources forms take
 * them since ABI version 4: heard links by the batch sweep, interference over the whole batch, rm_airbatch.hip), and their ticks */
int rm_air_batch_stats(const rm_context *ctx, uint64_t *batches, uint64_t *ticks);
/* observability (synchronises): the (heard link, frame on the air) pairs the last such batch evaluated exactly, the frames
 * its index held (on-air window + the batch's own), and how many of the pairs turned out to interfere */
int rm_air_batch_pairs(rm_context *ctx, uint64_t *pairs, uint64_t *frames, uint64_t *interferers);
/* the entry ring behind those lists (synchronises): entries allocated since the lists were last rebuilt in the busiest of the
 * 256 sub-rings, and the entries a sub-ring holds -- more allocated than held: the ring has gone round (old entries were reclaimed) */
int rm_air_ring_stats(rm_context *ctx, uint64_t *max_allocated, uint64_t *sub_ring_entries);

/* ---- channel energy query (CCA / ED) over the frames on the air ------------------------------------------
 * Not reference behaviour (the reference answers with the latched RSSI of a frame being received, or a constant:
 * Transciever.getRSSI, AbstractRadioMedium.getBaseRSSI -- rm_node_info mirrors that); the read side of the RM_LD_SINR
 * extension's state.  For node j, time t, channel c: a frame of the context's on-air window
 * counts iff its record is live (src >= 0), start_us <= t < start_us + air_us, channel == c, src != j and its rssi at j
 * (frame position from its record, node position from the table as it is now, shadowing as in E2) reaches ifloor_dbm;
 * energy_dbm = 10 log10(exact Q80 sum of the counting frames' linear powers + noise); no counting frame: the noise level.
 * flags: RM_ED_TRANSMITTING -- some live frame of j's own spans t, on any channel (the energy is still the sum over the
 * others); RM_ED_BUSY -- energy_dbm >= cca_threshold_dbm (a NaN threshold never sets it).  channel RM_CHANNEL_OWN: every
 * node on its own channel, else the given channel for every queried node.  The node's enabled / rxprob / txprob play no part.
 *
 * Frames get into the window through the lone ticks of every form (rm_tick_begin .. rm_tick_flush / rm_tick_run, rm_transmit,
 * rm_tick_run_sources_device, rm_tick_run_records_device) and through batches of overlapping ticks
 * (rm_batch_run_sources_device and the gathered-sources forms when frames outlive their tick).  A batch of self-contained
 * ticks leaves nothing of its earlier ticks: by its contract they have left the air when the next tick begins; with source
 * indices the LAST tick's frames stay in the window (they may outlive the batch), with records nothing does (the host cannot
 * see their spans) -- and such a batch does not move the clock the query is checked against.  A frame that had left the air
 * when a later tick began is gone for good.
 *
 * RM_ERR_STATE: the model is not RM_MODEL_LOGDIST with RM_LD_SINR (only that medium keeps frames on the air); between
 * rm_tick_begin and rm_tick_flush; a context with a receiver partition (rm_set_partition*), or whose window was selected
 * for a region (gathered batches over a partition) -- the rm_group_*, rm_dist_* and gathered forms are out of scope.
 * RM_ERR_INVALID: time_us earlier than the latest t_begin a tick over the window has had (frames that had left the air by
 * then are gone); a later time_us is fine: every frame's own span is tested and the window is not changed by a query; a
 * node index outside 0 .. n_nodes-1 in a host list (before anything is launched) -- in a device list such an entry gets
 * NaN energy and flags 0 and nothing else is disturbed.  An empty window is no error: the noise level everywhere.
 * Pending node changes are applied first, as a tick does.  The query writes the caller's outputs and scratch of its own,
 * nothing else: a tick, a batch or a drain after it gives what it gave without it. */
#define RM_CHANNEL_OWN (-1)
#define RM_ED_TRANSMITTING 1
#define RM_ED_BUSY 2
/* asynchronous on the context's stream; all pointers are device memory; dev_nodes NULL: nodes 0 .. n-1 */
int rm_channel_energy_device(rm_context *ctx, int64_t time_us, const int32_t *dev_nodes, int32_t n, int32_t channel,
                             double cca_threshold_dbm, double *dev_energy_dbm, uint8_t *dev_flags /* may be NULL */);
/* host arrays; synchronises; nodes NULL: nodes 0 .. n-1 */
int rm_channel_energy(rm_context *ctx, int64_t time_us, const int32_t *nodes, int32_t n, int32_t channel,
                      double cca_threshold_dbm, double *energy_dbm, uint8_t *flags /* may be NULL */);

/* ---- carrier-sense gated tick: candidates that find the channel busy defer, on the device --------------------
 * Listen before talk in one call (not reference behaviour).  A gated tick has candidates src[0..n)
 * (node indices, -1 = padding), one start_us and one air_us (as rm_tick_run_sources_device), a sample time cca_time_us and a
 * threshold cca_threshold_dbm.
 *  - For candidate i with src[i] = j >= 0, (energy_i, flags_i) is exactly the channel energy query above for node j at
 *    t = cca_time_us on j's own channel with that threshold, over the on-air window as it is when the tick begins: after the
 *    frames that had left the air by t_begin_us are gone and BEFORE any frame of this call joins it.  Candidates of one call
 *    never defer each other: they all start at the same instant, after the sample.
 *  - Candidate i is deferred iff flags_i != 0: RM_ED_BUSY (energy >= threshold) or RM_ED_TRANSMITTING (a frame of j's own
 *    spans cca_time_us: a radio cannot start a second frame).  A NaN threshold never sets BUSY: then only TRANSMITTING defers.
 *  - A deferred candidate becomes a padding record in its slot (what src = -1 means).  The tick is then, bit for bit, what
 *    rm_tick_run_sources_device gives for the list with those entries replaced by -1: packet numbers keep their positions, a
 *    deferred packet has an empty segment in pkt_offset, does not join the on-air window as a live frame, consumes no
 *    java.util.Random draw, and with the reception stage on it counts as a packet number but queues nothing.
 *  - Padding on input stays padding, with flags 0 and NaN energy.  The node's enabled / rxprob / txprob play no part in the
 *    sensing.
 * Refused before anything is launched, with nothing changed: RM_ERR_STATE under every condition under which
 * rm_channel_energy returns it (not RM_MODEL_LOGDIST with RM_LD_SINR, between rm_tick_begin and rm_tick_flush, a receiver
 * partition, a window selected for a region); RM_ERR_INVALID unless t_begin_us <= cca_time_us <= start_us (a sample may not
 * look back behind the latest t_begin of the window, and a sample after the start would have to see the call's own frames), and
 * for a host list entry outside -1 .. n_nodes-1 -- in a device list such an entry is treated as padding.
 * The caller's list is not written: the gated list lives in a buffer of the context.
 * The device form is asynchronous and deferral is padding -- no count comes back to the host -- so a host may issue many gated
 * lone ticks back to back without waiting.  A batch of ticks is gated by rm_batch_run_sources_cca* below.  One sample time per
 * tick: a sample time per candidate (the records forms) needs per-node span information that the per-query
 * RM_ED_TRANSMITTING stamp does not carry. */
/* asynchronous on the context's stream; all pointers device memory; outputs may be NULL */
int rm_tick_run_sources_cca_device(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us, const int32_t *dev_src, int32_t n,
                                   int64_t start_us, int64_t air_us, int64_t cca_time_us, double cca_threshold_dbm,
                                   uint8_t *dev_cca_flags /* [n] RM_ED_* */, double *dev_cca_energy_dbm /* [n] */);
/* host arrays in and out (outputs may be NULL); evaluates the tick, synchronises for the flags; results through rm_result_* as
 * after rm_tick_run_sources_device */
int rm_tick_run_sources_cca(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us, const int32_t *src, int32_t n, int64_t start_us,
                            int64_t air_us, int64_t cca_time_us, double cca_threshold_dbm, uint8_t *cca_flags, double *cca_energy_dbm);

/* ---- carrier-sense gated batch: listen before talk across a batch of ticks ------------------------------------
 * (not reference behaviour.)  The first eight arguments are those of rm_batch_run_sources_device;
 * cca_time_us[b] is tick b's sample time, t_begin_us[b] <= cca_time_us[b] <= start_us[b]; one threshold for the batch.  The
 * outputs are flat arrays of n_src[0] + ... + n_src[n_ticks-1] entries in tick order; either may be NULL.
 *  - For candidate i of tick b with src = j >= 0, (energy, flags) is the channel energy query for node j at t = cca_time_us[b]
 *    on j's own channel, over the on-air window as the batch finds it PLUS the kept frames of ticks 0 .. b-1 of this batch.  A
 *    candidate that an earlier tick deferred is not on the air: it is not sensed and does not set RM_ED_TRANSMITTING for its
 *    node.  Candidates of tick b itself never see each other.  Lists hold distinct nodes within a tick.
 *  - The candidate is deferred iff flags != 0, as in a gated lone tick.  Padding on input stays padding (flags 0, NaN energy); a
 *    device-list entry outside 0 .. n_nodes-1 is padding, in a host list it is RM_ERR_INVALID.
 *  - After the gate the call is, bit for bit, rm_batch_run_sources_device over the same arguments with every deferred entry
 *    replaced by -1: result slots, pkt_offset (an empty segment per deferred packet), the frames that join the window, and
 *    rm_events_process_batch afterwards.  The caller's lists are not written: the gated lists live in a buffer of the context.
 * It follows that a gated batch equals the same ticks issued as rm_tick_run_sources_cca* calls one by one, and any split into
 * smaller gated batches and gated lone ticks.
 * Refused before anything is launched, with the window unchanged: RM_ERR_STATE for everything rm_tick_run_sources_cca* refuses
 * with it, and for what rm_batch_run_sources_device refuses for the same arguments (links that can draw in a batch of
 * overlapping ticks, overlapping ticks out of time order, an unsorted receiver table, an overlapping tick of more than 8192
 * candidates, an fp64 frame); RM_ERR_INVALID for n_ticks outside
 * 1 .. RM_MAX_BATCH, a cca_time_us[b] outside [t_begin_us[b], start_us[b]] or behind the t_begin_us of an earlier tick of the
 * batch, a cca_time_us[0] behind the window's clock, an air time of 2^32 us or more, a bad host index.  (What only the sweep's
 * plan of a tick can tell -- a developer knob that takes the filter off its workgroup form -- is refused by the batch itself,
 * after the gate has run: the outputs are written, no frame joins the window.)
 * The device form waits once, inside the call, for the count that sizes the gate's pair list; everything else is asynchronous.
 * The gathered forms, rm_dist_* and rm_group_* are not gated. */
/* dev_src[b]: device memory; outputs device memory, may be NULL */
int rm_batch_run_sources_cca_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                    const int32_t *const *dev_src, const int32_t *n_src, const int64_t *start_us,
                                    const int64_t *air_us, const int64_t *cca_time_us, double cca_threshold_dbm,
                                    uint8_t *dev_cca_flags /* RM_ED_* */, double *dev_cca_energy_dbm);
/* host lists in, host arrays out (may be NULL); synchronises; results through rm_batch_result_* as after
 * rm_batch_run_sources_device */
int rm_batch_run_sources_cca(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                             const int32_t *const *src, const int32_t *n_src, const int64_t *start_us, const int64_t *air_us,
                             const int64_t *cca_time_us, double cca_threshold_dbm, uint8_t *cca_flags, double *cca_energy_dbm);

/* ---- CSMA-CA gated batch: a deferred candidate backs off and tries again, on the device -------------------------
 * (not reference behaviour.)  Unslotted CSMA-CA over the ticks of ONE gated batch.  Candidate k of
 * tick b is a PACKET with flat index o = n_src[0] + ... + n_src[b-1] + k, whatever its entry holds (a padding entry is a packet
 * that never attempts).  Attempt 0 of a packet is in tick b; if attempt a is made and deferred and a < max_backoffs, attempt
 * a + 1 is in tick T(a+1) = T(a) + 1 + r with BE = min(min_be + a, max_be), r = 0 if BE = 0 else h2 >> (64 - BE),
 * h1 = mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ uint64(cca_time_us[b])) (b: the ORIGIN tick), h2 = mix64(h1 ^ (uint64(k) << 8 | a)),
 * mix64 = the SplitMix64 finaliser of E2.  The schedule depends on the tick times, the list lengths and the parameters only:
 * rm_csma_schedule computes it without a device.
 *  - The EXPANDED list of tick T: its n_src[T] own entries, then every attempt a >= 1 of any packet with T(a) = T, ordered by
 *    (origin tick, origin slot); n_exp[T] entries.  Packet numbers of tick T are positions in that list.  Attempts that fall at
 *    T >= n_ticks are not part of the batch.
 *  - An attempt is MADE iff its entry is a node 0 .. n_nodes-1 and every earlier attempt of its packet was made and deferred;
 *    otherwise its slot is padding (nothing sensed).  A made attempt of node j in tick T is sensed exactly as a candidate of tick T
 *    of rm_batch_run_sources_cca*: the window as the batch finds it plus the KEPT frames of ticks 0 .. T-1.
 *  - One frame per radio per tick: among a node's slots of a tick with flags 0 the first in list order is kept; a later one gets
 *    RM_ED_TRANSMITTING or-ed into its flags and counts as deferred.  (This replaces E7's "distinct nodes within a tick", which
 *    a caller cannot guarantee for retries; the own lists still hold distinct nodes per tick.)
 *  - Per packet: RM_CSMA_NONE (padding entry; attempts 0, pkt -1), RM_CSMA_SENT (tick = the kept attempt's tick, pkt = its
 *    position in that tick's expanded list), RM_CSMA_FAILED (attempt max_backoffs made and deferred; pkt -1), RM_CSMA_PENDING (the
 *    next attempt falls at tick >= n_ticks; tick = that batch-relative tick, pkt -1).  attempts = attempts made; flags and
 *    energy_dbm are those of the last attempt made (0 and NaN if none).  tick is -1 where the table has none.
 *  - After the gate the call is, bit for bit, rm_batch_run_sources_device over the same tick times with n_exp and the gated
 *    expanded lists (result slots, pkt_offset, the frames that join the window, java.util.Random untouched,
 *    rm_events_process_batch afterwards).  The caller's lists are never written.  With max_backoffs = 0 the call is
 *    rm_batch_run_sources_cca* bit for bit.
 * Refused before anything is launched, window unchanged: everything rm_batch_run_sources_cca* refuses, with its codes (the
 * 8192-candidate limit of an overlapping tick applies to n_exp[T]); RM_ERR_INVALID for parameters out of range or reserved != 0.
 * A pending packet's chain ends with the batch; rm_batch_run_sources_csma_carry* below (E9) takes it into the next batch, and with it
 * any split into consecutive batches gives the result of the whole.  The gathered forms, rm_dist_* and rm_group_* are not gated. */
#define RM_CSMA_NONE 0
#define RM_CSMA_SENT 1
#define RM_CSMA_FAILED 2
#define RM_CSMA_PENDING 3
typedef struct rm_csma_params {
    int32_t max_backoffs; /* 0 .. 5: busy samples after the first before giving up (macMaxCSMABackoffs; 802.15.4 default 4) */
    int32_t min_be;       /* 0 .. max_be */
    int32_t max_be;       /* min_be .. 8 */
    int32_t reserved;     /* 0 */
    uint64_t seed;
} rm_csma_params;
typedef struct rm_csma_result { /* flat, one entry per packet (sum of n_src); any pointer may be NULL */
    uint8_t *status;
    uint8_t *attempts;
    int32_t *tick;
    int32_t *pkt;
    uint8_t *flags;
    double *energy_dbm;
} rm_csma_result;
void rm_csma_defaults(rm_csma_params *p); /* 4, 3, 5, 0, seed 0 */
/* pure host function, no device needed: n_exp[n_ticks]; origin[] (flat packet index) / attempt[] per expanded slot in tick order
 * (may be NULL; cap entries); *total = sum of n_exp even when cap is too small (then RM_ERR_CAPACITY) */
int rm_csma_schedule(const rm_csma_params *p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us, int32_t *n_exp,
                     int32_t *origin, uint8_t *attempt, int64_t cap, int64_t *total);
/* dev_src[b]: device memory; dev_out's pointers device memory; n_exp: host, [n_ticks], may be NULL.  Waits once inside the call, as
 * rm_batch_run_sources_cca_device */
int rm_batch_run_sources_csma_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                     const int32_t *const *dev_src, const int32_t *n_src, const int64_t *start_us,
                                     const int64_t *air_us, const int64_t *cca_time_us, double cca_threshold_dbm,
                                     const rm_csma_params *p, const rm_csma_result *dev_out, int32_t *n_exp);
/* host lists in, host arrays out; synchronises; results through rm_batch_result_* with n_exp[b] packets in tick b */
int rm_batch_run_sources_csma(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                              const int32_t *const *src, const int32_t *n_src, const int64_t *start_us, const int64_t *air_us,
                              const int64_t *cca_time_us, double cca_threshold_dbm, const rm_csma_params *p,
                              const rm_csma_result *out, int32_t *n_exp);

/* ---- CSMA-CA gated batch with a carry: pending packets go on in the next batch ------------------------------------
 * (not reference behaviour.)  rm_batch_run_sources_csma* plus a list of CARRIED packets: packets
 * of earlier batches whose next attempt was behind their batch's last tick (RM_CSMA_PENDING).  A carried packet is a packet like
 * any other: its attempt number `attempt` is in tick `tick` of THIS batch, and its later attempts follow E8's formula with h1 made of
 * origin_cca_time_us, k = origin_slot and the attempt number running on.
 *  - The EXPANDED list of tick T holds, in this order: the tick's own entries; the attempts of carried packets that fall at T, in
 *    carry-list order; the retries of this batch's own packets, in (origin tick, origin slot) order.
 *  - A carried packet's first attempt inside this batch is made unconditionally, its later ones iff all earlier ones in this batch
 *    were made and deferred.  Sensing is exactly E8's, and so is the one-frame-per-radio-per-tick rule: the first in list order
 *    wins.  Two carried packets of one node are allowed.
 *  - carried_out is flat with n_carry entries (device memory in the device form; any pointer may be NULL): status, tick (relative
 *    to this batch) and pkt as E8; attempts is the TOTAL, the attempts made before this batch included; flags and energy_dbm are
 *    those of the last attempt made in this batch.  A carried packet with tick >= n_ticks has no slot: RM_CSMA_PENDING, attempts =
 *    attempt, tick unchanged, pkt -1, flags 0, energy NaN.
 *  - With n_carry = 0 the call IS rm_batch_run_sources_csma*, bit for bit (those entry points are this call).
 * Refused before anything is launched, window unchanged: everything E8 refuses, with its codes (the 8192 limit of an overlapping
 * tick applies to n_exp[T], carried slots included; RM_ERR_CAPACITY for more than 2^27 packets and carried packets together);
 * RM_ERR_INVALID for n_carry < 0, n_carry > 0 with carry NULL, a node outside 0 .. n_nodes-1, an attempt outside 1 .. max_backoffs,
 * tick < 0, origin_slot < 0.
 * rm_csma_carry_collect* make the next batch's carry list from a batch's results: the RM_CSMA_PENDING carried packets in carry-in
 * order, then the RM_CSMA_PENDING own packets in flat order, each with tick - n_ticks and attempt = attempts (only status, attempts
 * and tick are read).  That order is part of the contract: it is what makes the next batch's expanded lists those of the unsplit batch.
 * THE PROMISE: a CSMA-CA batch over ticks 0 .. N-1 and any split of it into consecutive carry batches, each fed the collected
 * carry-out of the one before, sense the same attempts with the same result, put the same frames on the air in the same ticks,
 * give the same heard links (dst, verdict, rssi, sinr, bit for bit, in the same order), leave the same on-air window, and give
 * every packet the same final status, attempts, absolute tick, flags and energy bits -- a packet's final entry being that of the
 * part in which it stopped being pending, with flags and energy of the last part in which it made an attempt.
 * PACKET NUMBERS are the one difference.  E8 schedules every attempt of every packet, made or not: the whole batch keeps a padding
 * slot (nothing sensed, an empty segment in pkt_offset) for each later attempt of a packet that was sent already.  A carry holds
 * pending packets only, so in the part after a cut those dead slots of packets from before the cut do not exist: n_exp[T] of the
 * part is the whole's minus its dead slots of T, and pkt, the links' pkt column and pkt_offset count positions among the
 * surviving slots, whose order is the whole's. */
typedef struct rm_csma_carry {  /* 24 bytes; always a HOST array, in both forms */
    int64_t origin_cca_time_us; /* cca_time_us of the packet's ORIGIN tick (what its backoff hash h1 is made of) */
    int32_t origin_slot;        /* its position k in the origin tick's own list (>= 0) */
    int32_t node;               /* 0 .. n_nodes-1 */
    int32_t tick;               /* tick of its next attempt, relative to THIS batch; >= 0, may be >= n_ticks */
    int32_t attempt;            /* number of that attempt: 1 .. max_backoffs (= attempts made so far) */
} rm_csma_carry;
/* pure host function: rm_csma_schedule plus the carried packets; in origin[] a carried slot is n_pkt + its carry index */
int rm_csma_schedule_carry(const rm_csma_params *p, int32_t n_ticks, const int32_t *n_src, const int64_t *cca_time_us,
                           const rm_csma_carry *carry, int32_t n_carry, int32_t *n_exp, int32_t *origin, uint8_t *attempt, int64_t cap,
                           int64_t *total);
/* as rm_batch_run_sources_csma_device; dev_carried_out's pointers device memory, n_carry entries each */
int rm_batch_run_sources_csma_carry_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                           const int32_t *const *dev_src, const int32_t *n_src, const int64_t *start_us,
                                           const int64_t *air_us, const int64_t *cca_time_us, double cca_threshold_dbm,
                                           const rm_csma_params *p, const rm_csma_result *dev_out, int32_t *n_exp,
                                           const rm_csma_carry *carry, int32_t n_carry, const rm_csma_result *dev_carried_out);
/* as rm_batch_run_sources_csma; carried_out's pointers host arrays */
int rm_batch_run_sources_csma_carry(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                    const int32_t *const *src, const int32_t *n_src, const int64_t *start_us, const int64_t *air_us,
                                    const int64_t *cca_time_us, double cca_threshold_dbm, const rm_csma_params *p,
                                    const rm_csma_result *out, int32_t *n_exp, const rm_csma_carry *carry, int32_t n_carry,
                                    const rm_csma_result *carried_out);
/* host results and host lists, no device needed.  carry_out: cap entries; *count = the entries the carry-out holds, also when cap is
 * too small (then RM_ERR_CAPACITY, carry_out unspecified).  out / carried_out: status, attempts and tick have to be there unless the
 * table is empty. */
int rm_csma_carry_collect(int32_t n_ticks, const int32_t *const *src, const int32_t *n_src, const int64_t *cca_time_us,
                          const rm_csma_carry *carry, int32_t n_carry, const rm_csma_result *out, const rm_csma_result *carried_out,
                          rm_csma_carry *carry_out, int64_t cap, int64_t *count);
/* device results (as the device form wrote them) and device lists; carry and carry_out are host arrays.  Ordered on the context's
 * stream after the batch; synchronises once. */
int rm_csma_carry_collect_device(rm_context *ctx, int32_t n_ticks, const int32_t *const *dev_src, const int32_t *n_src,
                                 const int64_t *cca_time_us, const rm_csma_carry *carry, int32_t n_carry, const rm_csma_result *dev_out,
                                 const rm_csma_result *dev_carried_out, rm_csma_carry *carry_out, int64_t cap, int64_t *count);

/* ---- frame error model: delivery decided from SINR and frame length -----------------------------------------------
 * (not reference behaviour.)  Opt-in, on the RM_LD_SINR medium only.  Without it a heard
 * link is delivered iff sinr >= ld_capture_db, whatever the frame's length; with RM_EM_OQPSK_250K a link that is RM_DELIVERED
 * under everything else (Tx failure, capture, half duplex, the rxProbability draw) becomes RM_INTERFERED iff !(u < psr):
 *   psr  = (1 - ber)^(air_us / us_per_bit), ber = 8/15 * 1/16 * sum_{k=2..16} (-1)^k C(16,k) exp(20 s (1/k - 1)), s = 10^(sinr/10),
 *          in the operations and the order of E-math that DESIGN.md E10 writes down (rm_error_model_psr is that, on the host);
 *          ber is clamped to [0, 0.5]; a NaN sinr gives a NaN psr, which never delivers;
 *   u    = the uniform deviate of mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ start_us) ^ (src << 32 | dst)): a function of the
 *          frame (source node, start time), the receiver and the seed alone (rm_error_model_draw) -- not of packet numbers,
 *          ticks, slots or ranks, and no java.util.Random draw is consumed.
 * Nothing else of a result changes: sinr, rssi, dst, pkt_offset, pkt_interference, the on-air window, the energy query and the
 * gates (they read no verdict).  ld_capture_db keeps working as a floor; -inf leaves the curve alone.  The verdict of a frame at a
 * receiver does not depend on whether a lone tick, a batch, a gated batch or any split of a CSMA-CA run into carry batches
 * evaluated it: E9's promise holds with the model on.
 * The pass (one launch over the finished result; a batch: one launch over all of its slots) runs inside the evaluating call,
 * before anything reads verdicts: rm_transmit, rm_tick_begin .. rm_tick_flush / _view / rm_tick_run, rm_tick_run_sources_device,
 * rm_tick_run_records_device, rm_batch_run_sources_device (both kinds), rm_batch_run_device, the gated forms (E6 - E9), and the
 * reception stage behind all of them.  A lone tick with the model on writes its compact arrays at once (one more launch).
 * rm_set_error_model: RM_ERR_STATE unless the model is RM_MODEL_LOGDIST with RM_LD_SINR, and on a context made under RM_GRAPH=1
 * (the pass is not part of the captured sequence); RM_ERR_INVALID for an unknown kind, reserved != 0, or us_per_bit not finite
 * and > 0.  rm_set_model switches the error model off (RM_EM_NONE).  While a model is on, an evaluating call on a context with
 * a receiver partition (rm_set_partition*) and the gathered / rm_dist_* / rm_group_* forms are refused with RM_ERR_STATE before
 * anything is launched, the window unchanged.  With RM_EM_NONE (the default) nothing is launched and nothing changes. */
enum rm_error_model_kind { RM_EM_NONE = 0, RM_EM_OQPSK_250K = 1 };
typedef struct rm_error_model {
    int32_t kind;      /* enum rm_error_model_kind */
    int32_t reserved;  /* 0 */
    double us_per_bit; /* 4.0: 250 kbit/s */
    uint64_t seed;
} rm_error_model;
void rm_error_model_defaults(rm_error_model *e, int32_t kind); /* us_per_bit 4.0, seed 0 */
int rm_set_error_model(rm_context *ctx, const rm_error_model *e);
int rm_get_error_model(const rm_context *ctx, rm_error_model *out);
/* pure host functions, no device (built from csrc/rm_math.hpp by the host compiler, like rm_det_math); RM_EM_NONE: psr 1 */
double rm_error_model_psr(const rm_error_model *e, double sinr_db, int64_t air_us);
double rm_error_model_draw(const rm_error_model *e, int32_t src, int64_t start_us, int32_t dst);

/* ---- per-node traffic counters accumulated on the device -----------------------------------------------------------
 * (not reference behaviour.)  Opt-in, on every medium.  With statistics on, every evaluating
 * call ends with one more launch on the context's stream that adds the call's results to a table of one rm_node_stats per node
 * index -- behind the frame error model's pass, so it counts the verdicts every result reader sees.  For every evaluated tick,
 * with its new frames q (record tx[q]: src, air_us) and its heard links i (packet q_i, receiver dst_i, final verdict v_i):
 *   a frame counts on the transmitter side iff 0 <= src_q < n_nodes (padding, deferred candidates of the gates and CSMA-CA slots
 *   not made are -1 and count nothing); then tx_frames[src_q] += 1, tx_air_us[src_q] += air_us_q, tx_failed[src_q] += pkt_interference[q];
 *   a heard link adds 1, air_us_{q_i} and [v_i == RM_DELIVERED] to rx_heard, rx_air_us and rx_delivered of dst_i, and, if its frame
 *   counts, 1 and [v_i == RM_DELIVERED] to tx_links_heard and tx_links_delivered of src_{q_i}.
 * rx_air_us is a sum per heard frame, not the union of their spans: frames that overlap at a receiver count twice.  Frames of
 * earlier ticks that are still on the air get no verdicts in a later tick and are never counted twice.  A tick whose result
 * overflowed the link capacity or was dropped counts nothing and adds 1 to ticks_skipped; every other non-empty tick adds 1 to
 * ticks_counted; an empty tick changes nothing.  All sums are integers: the table after any sequence of calls is the sum over
 * its ticks, whether they ran as lone ticks, a batch, a gated batch, a CSMA-CA batch or any split of a CSMA-CA run into carry
 * batches (nothing here is indexed by packet number).
 * Accepted on a whole-table context by rm_transmit, rm_tick_flush / _view / rm_tick_run, rm_tick_run_device,
 * rm_tick_run_sources_device, rm_tick_run_records_device, rm_batch_run_sources_device (both SINR kinds), rm_batch_run_device and
 * the gated forms (E6 - E9).  While statistics are on, an evaluating call on a context with a receiver partition
 * (rm_set_partition*) and the gathered / rm_dist_* / rm_group_* forms are refused with RM_ERR_STATE before anything is launched,
 * the on-air window unchanged; rm_stats_enable(ctx, 1) is RM_ERR_STATE on a context made under RM_GRAPH=1 (the pass is not part
 * of the captured sequence).  With statistics on, rm_transmit on a reference medium does not take its one-launch shortcut (whose
 * links never become a slot's result) but the general tick path: the links it returns are the same.  A lone tick with statistics
 * on writes its compact arrays at once (a dense tick: its records from the lane masks).
 * The counters do not depend on the medium: rm_set_model, rm_set_error_model, rm_seed, rm_node_update and rm_nodes_move keep them
 * and counting goes on.  rm_nodes_upload with the same node count keeps them; another node count resizes the table and zeroes it
 * and the totals (pointers handed out by rm_stats_device are stale then).  With statistics off (the default) nothing is launched
 * and nothing allocated. */
typedef struct rm_node_stats {
    uint64_t tx_frames;          /* frames this node put on the air */
    uint64_t tx_failed;          /* of those, frames whose per-packet Tx-failure flag (pkt_interference) is set */
    uint64_t tx_air_us;          /* sum of air_us of those frames */
    uint64_t tx_links_heard;     /* heard links of those frames */
    uint64_t tx_links_delivered; /* of those, links whose final verdict is RM_DELIVERED */
    uint64_t rx_heard;           /* heard links with this node as receiver */
    uint64_t rx_delivered;       /* of those, RM_DELIVERED */
    uint64_t rx_air_us;          /* sum of air_us of the frames of those heard links (per heard frame: overlapping frames count twice) */
} rm_node_stats;                 /* 64 bytes */
typedef struct rm_stats_totals { uint64_t ticks_counted, ticks_skipped; } rm_stats_totals;
/* on = 1: allocate the table (zeroed) if need be and count from the next evaluating call; 0: stop counting, the table is kept */
int rm_stats_enable(rm_context *ctx, int32_t on);
int rm_stats_enabled(const rm_context *ctx);
/* zero the table and the totals, on the context's stream.  RM_ERR_STATE before the first rm_stats_enable(ctx, 1), as the next two. */
int rm_stats_reset(rm_context *ctx);
/* the listed nodes' records in list order (nodes == NULL: all, in node order; n has to be the node count then), and the totals
 * (or NULL).  Synchronises the context's stream once.  RM_ERR_INVALID: an index outside 0 .. n_nodes - 1. */
int rm_stats_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_node_stats *out, rm_stats_totals *totals);
/* the table ([n_nodes], by node index) and the totals in device memory: valid until statistics are enabled with another node
 * count (or rm_nodes_upload changes it) or the context is destroyed; the caller's reads are ordered by the context's stream */
int rm_stats_device(rm_context *ctx, const rm_node_stats **dev_table, const rm_stats_totals **dev_totals);

/* ---- unicast outcome query: did a frame reach its destination -------------------------------------------------------
 * (not reference behaviour.)  The medium is broadcast: a result lists every receiver that
 * heard a frame.  The query answers, on the device and over the FINISHED results of the last evaluating call, what became of a
 * frame at the one node it was addressed to.  A query entry names a result slot b (tick b of the last batch; slot 0 is also the
 * last lone tick, as rm_result_* reads it), a packet number p in that slot and a wanted node w.  With n_new(b) the slot's new
 * frames, rec = tx[first_new + p] the frame's record and [lo, hi) = [pkt_offset[p], pkt_offset[p + 1]) its segment of heard links
 * (dst ascends inside it), the FIRST rule that applies gives the entry's status:
 *   RM_UC_NONE        w < 0, b < 0, b >= slots of the last call, p < 0 or p >= n_new(b): nothing asked, or no such packet (a CSMA-CA
 *                     packet that was not sent has tick / pkt -1);
 *   RM_UC_LOST        the slot overflowed its link capacity or was dropped (what the traffic counters skip);
 *   RM_UC_NOT_SENT    rec.src outside 0 .. n_nodes-1 (padding, a candidate a gate deferred, a CSMA-CA slot not made);
 *   RM_UC_UNHEARD     no link i in [lo, hi) with dst[i] == w (so for w == rec.src, and for w >= n_nodes in a device list);
 *   RM_UC_INTERFERED  that link exists and its final verdict is not RM_DELIVERED;
 *   RM_UC_DELIVERED   that link exists and its final verdict is RM_DELIVERED.
 * Final: after the draws, the SINR stages and the frame error model's pass -- what every result reader sees.  Outputs per entry
 * (rm_unicast_out; any pointer may be NULL): status; link = i, the link's index into the slot's arrays, for the last two and -1
 * otherwise; rssi and sinr bit for bit what rm_result_copy / rm_batch_result_copy give at that index, NaN without a link, sinr NaN
 * on media without the SINR column; reply_src = w where the frame was delivered and -1 otherwise -- the list has the shape of a
 * source list and can be handed to rm_tick_run_sources_device as it lies in device memory (the acknowledgement tick).  It names a
 * node twice when two packets were delivered to the same destination: that is the caller's business.
 * status, rssi bits and sinr bits of a frame at its wanted receiver do not depend on whether a lone tick, a batch, a gated batch, a
 * CSMA-CA batch or any split of a CSMA-CA run into carry batches evaluated it; link is a position and may differ.
 * The query only reads: results, the on-air window and the generator are never touched, and nothing is launched before a refusal.
 * RM_ERR_STATE: no evaluated result yet; a context with a receiver partition (links of other ranks are not there); after a gathered
 * / rm_dist_* / rm_group_* call; a context made under RM_GRAPH=1.  RM_ERR_INVALID: NULL arguments, negative counts, n_slots outside
 * 1 .. slots of the last call, n_pkt[b] < 0, a want >= n_nodes in a HOST list.  RM_ERR_CAPACITY: more than 2^27 entries.
 * The device forms enqueue on the context's stream and do not wait: the outputs are valid when the stream reaches them.  The host
 * forms synchronise the stream once.  The slots are read as they are until the next evaluating call. */
enum rm_unicast_status { RM_UC_NONE = 0, RM_UC_NOT_SENT = 1, RM_UC_UNHEARD = 2, RM_UC_INTERFERED = 3, RM_UC_DELIVERED = 4, RM_UC_LOST = 5 };
typedef struct rm_unicast_out { uint8_t *status; int32_t *link; double *rssi; double *sinr; int32_t *reply_src; } rm_unicast_out; /* any may be NULL */
/* packets 0 .. n_pkt[b]-1 of slots 0 .. n_slots-1, flat in slot order; n_pkt is a host array (entries past a slot's packets: RM_UC_NONE) */
int rm_unicast_query_device(rm_context *ctx, int32_t n_slots, const int32_t *n_pkt, const int32_t *dev_want, const rm_unicast_out *dev_out);
int rm_unicast_query(rm_context *ctx, int32_t n_slots, const int32_t *n_pkt, const int32_t *want, const rm_unicast_out *out);
/* entry e names (slot[e], pkt[e]): exactly the tick / pkt columns of rm_csma_result (own or carried packets) */
int rm_unicast_query_at_device(rm_context *ctx, int64_t n, const int32_t *dev_slot, const int32_t *dev_pkt, const int32_t *dev_want,
                               const rm_unicast_out *dev_out);
int rm_unicast_query_at(rm_context *ctx, int64_t n, const int32_t *slot, const int32_t *pkt, const int32_t *want, const rm_unicast_out *out);
/* pure host function, no device (like rm_csma_carry_collect): the same answer from one tick's host result, packets 0 .. r->n_packets-1.
 * src[n_packets] may be NULL (every packet sent); reads pkt_offset, dst, verdict, rssi or pkt_rssi, sinr (NULL: NaN); r->count /
 * capacity problems are the caller's (no RM_UC_LOST).  RM_ERR_INVALID: NULL r / want / out, n_nodes < 0, a want >= n_nodes. */
int rm_unicast_from_result(const rm_host_result *r, const int32_t *src, int32_t n_nodes, const int32_t *want, const rm_unicast_out *out);

/* ---- receiver listening schedules: duty-cycled radios on the device ------------------------------------------------
 * (not reference behaviour.)  Opt-in, on every medium.  One rm_listen_schedule per node
 * index, a table of the context (like the traffic counters').  period_us = 0: the radio always listens (the default of every
 * node; on_us and phase_us have to be 0 then).  period_us > 0: 0 <= on_us <= period_us and 0 <= phase_us < period_us.
 * listening(s, t): 1 when s.period_us == 0; otherwise d = int64(uint64(t) - uint64(s.phase_us)) (a wrapping subtraction),
 * r = d % s.period_us in C semantics, if (r < 0) r += s.period_us, and listening = r < s.on_us -- so on_us = 0 never listens and
 * on_us = period_us always does.
 * With schedules on, every evaluating call ends with one more pass over its finished result, behind the frame error model's pass
 * and ahead of the traffic counters': a link whose verdict is RM_DELIVERED under everything else (Tx failure, capture, half
 * duplex, the rxProbability draw, the error model) becomes RM_INTERFERED iff !listening(sched[dst], rec.start_us), rec =
 * tx[first_new + pkt] the frame's own record -- the radio is sampled at the frame's first microsecond -- and missed[dst] += 1
 * (uint64 per node: links that everything else had delivered and that sleep alone lost).  Nothing else changes: dst, rssi, sinr,
 * pkt_offset, pkt_interference, the on-air window and java.util.Random are as with the feature off (a link at a sleeping receiver
 * still consumes its draw; this is NOT setEnabled(false), which takes the receiver out of the sweep); the energy query and the
 * gates (E5 - E9) ignore schedules (a CCA sample switches the radio on; the transmitter's own schedule plays no part).  A slot
 * that overflowed its link capacity or was dropped is left as it is and counts nothing.  The traffic counters and the unicast
 * query see the verdict after this pass.  A frame's verdict at a receiver and the missed table do not depend on whether a lone
 * tick, a batch, a gated batch, a CSMA-CA batch or any split of a CSMA-CA run into carry batches evaluated it; with every
 * period 0 the results are bit for bit those with the feature off.
 * Accepted by every evaluating call the traffic counters accept, on a whole-table context.  With schedules on, rm_transmit on a
 * reference medium takes the general tick path (same links), a lone tick writes its compact arrays at once, and a dense tick ends
 * with its records: rm_result_dense is RM_ERR_STATE for it (one verdict per packet cannot express the pass).  Refused with
 * RM_ERR_STATE before anything is launched, window, generator and tables untouched: contexts with a receiver partition, the
 * gathered / rm_dist_* / rm_group_* forms; rm_listen_set on a context made under RM_GRAPH=1.
 * rm_set_model, rm_seed, rm_node_update, rm_nodes_move and rm_nodes_upload with the same node count keep both tables;
 * rm_nodes_upload with another node count clears the feature as rm_listen_clear does.  Off (the default): nothing is launched. */
typedef struct rm_listen_schedule { int64_t period_us; int64_t on_us; int64_t phase_us; } rm_listen_schedule; /* 24 bytes */
/* nodes == NULL: sched[n] for all nodes in node order, n has to be the node count; otherwise sched[k] for node nodes[k], applied in
 * list order (the last entry of a node wins).  The whole list is validated before anything changes (RM_ERR_INVALID: a bad record, an
 * index outside 0 .. n_nodes - 1, NULL arguments, a negative count).  Switches the feature on; ordered on the context's stream:
 * it applies to calls evaluated after it. */
int rm_listen_set(rm_context *ctx, const int32_t *nodes, int32_t n, const rm_listen_schedule *sched);
/* the schedules of the listed nodes (the same list convention).  RM_ERR_STATE before the first rm_listen_set, as the calls below. */
int rm_listen_get(rm_context *ctx, const int32_t *nodes, int32_t n, rm_listen_schedule *out);
/* switches the feature off: every node always listens, missed is zeroed, nothing is launched afterwards */
int rm_listen_clear(rm_context *ctx);
int rm_listen_enabled(const rm_context *ctx);
/* missed of the listed nodes in list order (nodes == NULL: all, n has to be the node count).  Synchronises the stream once. */
int rm_listen_missed_read(rm_context *ctx, const int32_t *nodes, int32_t n, uint64_t *out);
/* zeroes missed, on the context's stream */
int rm_listen_missed_reset(rm_context *ctx);
/* both tables ([n_nodes], by node index) in device memory: valid until rm_listen_clear, another node count or rm_destroy; the
 * caller's reads are ordered by the context's stream */
int rm_listen_device(rm_context *ctx, const rm_listen_schedule **dev_sched, const uint64_t **dev_missed);
/* the listening rule itself, a pure host function without a device: 1, 0, or RM_ERR_INVALID for a NULL or bad record */
int rm_listen_at(const rm_listen_schedule *s, int64_t t_us);

/* ---- watched-link statistics: per-link counters on the device -------------------------------------------------------
 * (not reference behaviour.)  Opt-in, on every medium.  What a link estimator reads (ETX / PRR
 * over beacons, neighbour time-outs) without copying heard links to the host: every node has K slots of watched peers, set by the
 * caller, and one rm_link_stats per (node, slot).  Two tables of the context, both [n_nodes][K] in device memory: peer (int32,
 * -1: an empty slot) and the entries; and one rm_stats_totals.  K is 1, 2, 4 or 8 (a power of two: a node's peer row is one
 * aligned load of 4 K bytes).  A cleared entry is {0, 0, 0, 0, INT64_MAX, INT64_MIN}.
 * With the feature on, every evaluating call ends with one more pass over its finished result, behind the frame error model's,
 * the listening schedules' and the traffic counters' passes (E10, E13, E11, then this).  A slot that is empty changes nothing; one
 * that overflowed its link capacity or was dropped adds nothing and ticks_skipped += 1 (the traffic counters' conditions); every
 * other one ticks_counted += 1, and for every heard link i of it, with rec = tx[first_new + pkt[i]], s = rec.src, j = dst[i]: if
 * s and j are node indices and peer[j][k] == s for some k, entry (j, k) gets heard += 1; delivered += 1 iff the link's final
 * verdict (after the draws, the SINR stages, E10's and E13's passes) is RM_DELIVERED; rssi_q8_sum += q8(rssi[i]); sinr_q8_sum +=
 * q8(sinr[i]) on a medium with the sinr column (elsewhere it stays 0); first_start_us = min(first_start_us, rec.start_us);
 * last_start_us = max(last_start_us, rec.start_us).  q8(x) = 0 unless fabs(x) < 2147483648.0 (so NaN and the infinities give 0),
 * otherwise (int64_t)floor(x * 256.0 + 0.5), one rounding per operation and no fma: rm_linkstats_q8.  Nothing else is read or
 * written: results, the on-air window, java.util.Random, the traffic counters and the listening schedules' tables are as with the
 * feature off.  All sums are integers, minima or maxima: the tables after any sequence of calls do not depend on whether lone
 * ticks, a batch, a gated batch, a CSMA-CA batch or any split of a CSMA-CA run into carry batches evaluated the frames.
 * Peers are the caller's: this pass inserts and evicts nothing by what is heard (the neighbour tables below, rm_nbtable_*, do).
 * Accepted and refused where the traffic counters are: every evaluating call on a whole-table context (a dense tick ends with its
 * records and rm_result_dense keeps answering; rm_transmit on a reference medium takes the general tick path); refused with
 * RM_ERR_STATE before anything is launched, window, generator and tables untouched: contexts with a receiver partition, the
 * gathered / rm_dist_* / rm_group_* forms; rm_linkstats_enable(ctx, K > 0) on a context made under RM_GRAPH=1.
 * rm_set_model, rm_seed, rm_node_update, rm_nodes_move and rm_nodes_upload with the same node count keep the tables;
 * rm_nodes_upload with another node count switches the feature off.  Off (the default): nothing is launched, nothing allocated.
 * Memory: n_nodes * K * 52 bytes (416 MB at a million nodes and K = 8). */
typedef struct rm_link_stats {
    uint64_t heard;          /* heard links from the watched peer at this node */
    uint64_t delivered;      /* of those, links whose final verdict is RM_DELIVERED */
    int64_t rssi_q8_sum;     /* sum of q8(rssi) over the heard links: dBm in 1/256 */
    int64_t sinr_q8_sum;     /* sum of q8(sinr) over the heard links (0 on a medium without the sinr column) */
    int64_t first_start_us;  /* smallest start_us of a heard frame; INT64_MAX: none yet */
    int64_t last_start_us;   /* largest start_us of a heard frame; INT64_MIN: none yet */
} rm_link_stats;             /* 48 bytes */
/* K = 1, 2, 4 or 8: switches the feature on with K slots per node, every slot empty, every entry cleared, the totals 0; the same K
 * again changes nothing, another K starts from empty tables.  K = 0: off, the tables released.  Any other K: RM_ERR_INVALID. */
int rm_linkstats_enable(rm_context *ctx, int32_t K);
/* K, or 0 while the feature is off */
int rm_linkstats_enabled(const rm_context *ctx);
/* peers is n x K, row-major: row r for node nodes[r] (nodes == NULL: for all nodes in node order, n has to be the node count).  A
 * row's entry is -1 or a node index 0 .. n_nodes - 1 other than the row's own node; the non-negative entries of a row are
 * distinct; a node appears at most once in nodes.  The whole list is validated before anything changes (RM_ERR_INVALID).  A slot
 * whose peer stays as it was keeps its entry; a slot whose peer changes gets a cleared entry.  Ordered on the context's stream:
 * it applies to calls evaluated after it.  RM_ERR_STATE while the feature is off, as the four calls below. */
int rm_linkstats_watch(rm_context *ctx, const int32_t *nodes, int32_t n, const int32_t *peers);
/* the peer rows of the listed nodes (the same list convention), n x K */
int rm_linkstats_peers_get(rm_context *ctx, const int32_t *nodes, int32_t n, int32_t *out);
/* the entries of the listed nodes, n x K, and the totals (or NULL).  Synchronises the context's stream once. */
int rm_linkstats_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_link_stats *out, rm_stats_totals *totals);
/* clears every entry and the totals and keeps the peers, on the context's stream */
int rm_linkstats_reset(rm_context *ctx);
/* the three tables in device memory: valid until the feature is switched off or enabled with another K, another node count or
 * rm_destroy; the caller's reads are ordered by the context's stream */
int rm_linkstats_device(rm_context *ctx, const int32_t **dev_peer, const rm_link_stats **dev_table, const rm_stats_totals **dev_totals);
/* q8 itself, a pure host function without a device */
int64_t rm_linkstats_q8(double x);
/* the validation of rm_linkstats_watch alone, a pure host function without a device: RM_OK or RM_ERR_INVALID */
int rm_linkstats_validate(int32_t n_nodes, int32_t K, const int32_t *nodes, int32_t n, const int32_t *peers);

/* ---- traffic schedules: periodic sources generated on the device ----------------------------------------------------
 * (not reference behaviour.)  Opt-in.  One rm_traffic_schedule per node index, a table of the
 * context.  period_us = 0: the node generates nothing (the default of every node; the other fields have to be 0 then).  Otherwise
 * 1 <= period_us <= 2^40, 0 <= phase_us < period_us, 0 <= jitter_us <= period_us, reserved = 0.
 * Node i with P = period_us > 0 has packets k = 0, 1, 2, ...: due(i, k) = phase_us + k * P + j(i, k); j = 0 when jitter_us = 0,
 * otherwise j = (h * uint64(jitter_us)) >> 64 (the high half of the 128-bit product), h = mix64(mix64(mix64(seed +
 * 0x9E3779B97F4A7C15) ^ uint64(uint32(i))) ^ uint64(k)), mix64 the finaliser of E2.  jitter_us <= period_us, so due grows
 * strictly with k; jitter_us = period_us is "once per period at a uniformly random instant".
 * The generator turns the table, for n_ticks (1 .. RM_MAX_BATCH) half-open windows [win_lo[b], win_hi[b]) (host arrays; 0 <=
 * win_lo[b] <= win_hi[b] <= 2^62, win_hi[b] <= win_lo[b + 1]: in time order and disjoint, gaps and empty windows allowed), into
 * the per-tick source lists the batch calls take: node i is a source of window b iff one of its packets has win_lo[b] <= due <
 * win_hi[b].  Row b of src (int32[n_ticks][cap]) holds those nodes in ascending node index -- distinct, as the gated and CSMA-CA
 * batches require of a tick's own list -- padded with -1 up to cap; count[b] is the true number of sources; with count[b] > cap the
 * row holds the first cap of them in node order.  The windows are the generator's own arguments: it does not interpret the
 * engine's t_begin / t_end / start_us, and a due time inside a window is quantised to whatever start_us the caller gives that
 * tick.  A node's enabled flag, txprob and channel play no part.  Totals: packets = packets due in any window; coalesced = packets
 * minus the (node, window) pairs (second and later packets of a node in one window); truncated = the sum over b of max(0,
 * count[b] - cap).  The result is a pure function of (table, seed, windows, cap): the packets, and so the union of the lists, over
 * any partition of a time span into windows and into calls are the same; nothing depends on launch geometry, batch size or call
 * order, and no state is carried between calls.
 * No evaluating call changes, and the generator reads only its own table: it is accepted on partitioned contexts too (every rank
 * gets the same lists).  rm_set_model, rm_seed, rm_node_update, rm_nodes_move and rm_nodes_upload with the same node count keep
 * the table; rm_nodes_upload with another node count clears the feature as rm_traffic_clear does.  Off (the default): nothing is
 * allocated or launched. */
typedef struct rm_traffic_schedule { int64_t period_us; int64_t phase_us; int64_t jitter_us; int64_t reserved; } rm_traffic_schedule; /* 32 bytes */
typedef struct rm_traffic_totals { uint64_t packets; uint64_t coalesced; uint64_t truncated; } rm_traffic_totals;
/* nodes == NULL: sched[n] for all nodes in node order, n has to be the node count; otherwise sched[k] for node nodes[k], applied in
 * list order (the last entry of a node wins).  The whole list is validated before anything changes (RM_ERR_INVALID: a bad record, an
 * index outside 0 .. n_nodes - 1, NULL arguments, a negative count).  Switches the feature on; ordered on the context's stream.
 * RM_ERR_STATE on a context made under RM_GRAPH=1. */
int rm_traffic_set(rm_context *ctx, const int32_t *nodes, int32_t n, const rm_traffic_schedule *sched);
/* the schedules of the listed nodes (the same list convention), read from the device's table; synchronises the stream once.
 * RM_ERR_STATE before the first rm_traffic_set and after rm_traffic_clear, as rm_traffic_device and the generator. */
int rm_traffic_get(rm_context *ctx, const int32_t *nodes, int32_t n, rm_traffic_schedule *out);
/* switches the feature off: the table is forgotten */
int rm_traffic_clear(rm_context *ctx);
int rm_traffic_enabled(const rm_context *ctx);
/* the table ([n_nodes], by node index) in device memory: valid until rm_traffic_clear, another node count or rm_destroy; the
 * caller's reads are ordered by the context's stream.  RM_ERR_INVALID for a NULL dev_sched. */
int rm_traffic_device(rm_context *ctx, const rm_traffic_schedule **dev_sched);
/* The generator, enqueued on the context's stream without waiting for it: dev_src int32[n_ticks][cap], dev_count int32[n_ticks],
 * dev_totals one rm_traffic_totals or NULL, all device memory.  Row b is a ready source list of rm_batch_run_sources_device and the
 * gated forms: dev_src + b * cap with n_src[b] = count[b], or, without reading count back, with n_src[b] = cap (-1 entries are
 * padding there).  RM_ERR_INVALID: NULL arguments, n_ticks outside 1 .. RM_MAX_BATCH, cap < 1, windows that break the rule above;
 * RM_ERR_CAPACITY: n_ticks * cap above 2^27. */
int rm_traffic_generate_device(rm_context *ctx, uint64_t seed, int32_t n_ticks, const int64_t *win_lo, const int64_t *win_hi, int32_t cap,
                               int32_t *dev_src, int32_t *dev_count, rm_traffic_totals *dev_totals);
/* the same into host arrays (src int32[n_ticks][cap], count int32[n_ticks], totals or NULL); synchronises the stream once */
int rm_traffic_generate(rm_context *ctx, uint64_t seed, int32_t n_ticks, const int64_t *win_lo, const int64_t *win_hi, int32_t cap,
                        int32_t *src, int32_t *count, rm_traffic_totals *totals);
/* due(node, k) itself, a pure host function without a device: 1 and *due_us; 0 for period_us 0 (no packets); RM_ERR_INVALID for a
 * NULL or bad record, NULL due_us, node < 0, k < 0 or k * period_us above 2^62 (no window reaches such a packet) */
int rm_traffic_due(const rm_traffic_schedule *s, uint64_t seed, int32_t node, int64_t k, int64_t *due_us);
/* the validation of rm_traffic_set alone, a pure host function without a device: RM_OK or RM_ERR_INVALID */
int rm_traffic_validate(int32_t n_nodes, const int32_t *nodes, int32_t n, const rm_traffic_schedule *sched);

/* ---- neighbour query: each node's K strongest potential links on the device -------------------------------------------
 * (not reference behaviour.)  A pure function of the node table and the model, on
 * RM_MODEL_LOGDIST only (with or without RM_LD_SINR; the flag plays no part): the reference's media report the frame's txpower as
 * every link's rssi, a ranking by it says nothing there.
 * The potential link s -> r exists iff r != s, r's radio is enabled, r's channel is s's, !(rxprob_r <= 0) and rssi >=
 * sensitivity_dbm, rssi being the log-distance medium's value (shadowing included) for the Tx record rm_tick_run_sources_device
 * builds for s from the table: exactly the heard links of a lone tick whose only source is s, with their rssi bit for bit.  A NaN
 * rssi is no link; s's enabled flag and txprob and every verdict-side quantity play no part.
 * Link a precedes link b iff rssi_a > rssi_b, or rssi_a == rssi_b (as doubles) and a's far end has the lower node index.
 * RM_NB_HEARD_BY: the queried node j transmits, its row holds the receivers that hear it best.  RM_NB_HEARS: j receives, its row
 * holds the transmitters it hears best, each with its own table txpower -- the row a watch of rm_linkstats wants.
 * Per queried entry e, with 1 <= K <= RM_NB_MAX_K: peer[e][0 .. K) the far ends of the first K links in that order, padded with -1;
 * rssi[e][0 .. K) those links' rssi, the NaN 0x7FF8000000000000 beside a -1 (may be NULL); degree[e] the number of ALL potential
 * links of j in that direction, not capped at K (may be NULL).  Nothing is changed by a query. */
#define RM_NB_HEARD_BY 0
#define RM_NB_HEARS 1
#define RM_NB_MAX_K 16
/* Enqueued on the context's stream without waiting for it; all arrays are device memory.  dev_nodes == NULL: all nodes in index
 * order, n has to be the node count; otherwise entry e is node dev_nodes[e], and an entry outside 0 .. n_nodes - 1 gives a row of -1
 * and degree 0 and disturbs nothing else.  RM_ERR_STATE, nothing launched: another medium than RM_MODEL_LOGDIST, between
 * rm_tick_begin and rm_tick_flush, a context with a receiver partition, a context made under RM_GRAPH=1.  RM_ERR_INVALID: NULL ctx
 * or dev_peer, K outside 1 .. RM_NB_MAX_K, an unknown direction, n < 0, dev_nodes == NULL with n != n_nodes.  RM_ERR_CAPACITY:
 * n * K above 2^27.  n == 0 is RM_OK. */
int rm_neighbors_query_device(rm_context *ctx, int32_t direction, int32_t K, const int32_t *dev_nodes, int32_t n, int32_t *dev_peer,
                              double *dev_rssi, int32_t *dev_degree);
/* the same with host arrays; a node index outside the table is RM_ERR_INVALID before anything is launched.  Synchronises once. */
int rm_neighbors_query(rm_context *ctx, int32_t direction, int32_t K, const int32_t *nodes, int32_t n, int32_t *peer, double *rssi,
                       int32_t *degree);
/* The same order applied to the heard links of the first n_pkt packets of one tick's host result, a pure host function without a
 * device: peer / rssi [n_pkt][K], degree [n_pkt] (rssi and degree may be NULL).  These are the RM_NB_HEARD_BY rows of the packets'
 * sources when every packet is a distinct source alone in its tick's channel.  RM_ERR_INVALID: NULL r or peer, K outside
 * 1 .. RM_NB_MAX_K, n_pkt < 0 or above r->n_packets, a result with links but without pkt_offset, dst or an rssi column. */
int rm_neighbors_from_result(const rm_host_result *r, int32_t n_pkt, int32_t K, int32_t *peer, double *rssi, int32_t *degree);
/* rm_linkstats_watch with the list and the rows in device memory (dev_nodes == NULL: all nodes, n has to be the node count;
 * dev_peers n x K of the enabled K): rm_linkstats_validate's rules are checked by one launch on the device and its flag is waited
 * for -- RM_ERR_INVALID with nothing changed -- then the rows are applied as rm_linkstats_watch applies them.  An RM_NB_HEARS
 * result with the same K is valid by construction.  RM_ERR_STATE while the feature is off. */
int rm_linkstats_watch_device(rm_context *ctx, const int32_t *dev_nodes, int32_t n, const int32_t *dev_peers);
/* a block of device memory the context owns with room for n_nodes x K rows, for a caller without a device allocator of its own:
 * rm_neighbors_query_device writes there, rm_linkstats_watch_device reads from there.  Valid until the feature is switched off or
 * enabled with another K, another node count or rm_destroy; a whole-table rm_linkstats_watch overwrites it.  RM_ERR_STATE while
 * the feature is off. */
int rm_linkstats_stage_device(rm_context *ctx, int32_t **dev_rows);

/* ---- hop query: hop count and best parent toward a set of roots --------------------------------------------------------
 * (not reference behaviour.)  A pure function of the node table and the model, on
 * RM_MODEL_LOGDIST only (with or without RM_LD_SINR; the flag plays no part): whom a node addresses in a collection or a
 * dissemination tree, without the host seeing a link.
 * link(j, p, dir) holds iff p is a far end of j's potential links in direction dir exactly as the neighbour query defines them
 * (RM_NB_HEARD_BY: j transmits and p receives; RM_NB_HEARS: p transmits with its own table txpower and j receives; the table as it
 * is now, shadowing, enabled, channel and rxprob of the receiving end; a NaN rssi is no link) and rssi >= min_rssi_dbm, rssi being
 * that link's value of the neighbour query.  min_rssi_dbm = -inf keeps every potential link, +inf none; rssi == min_rssi_dbm is a
 * link.  direction is the link between a node and its parent, seen from the node: RM_NB_HEARD_BY gives a collection tree (the
 * node is heard by its parent), RM_NB_HEARS a dissemination tree (the node hears its parent).
 * hop[r] = 0 for every root r, whatever its radio state; for L = 0, 1, ... an unlabelled node j gets hop[j] = L + 1 iff
 * link(j, p, dir) for some p with hop[p] = L; a node never labelled has hop -1.  For hop[j] = h >= 1, parent[j] is, among all p
 * with hop[p] = h - 1 and link(j, p, dir), the first in the neighbour query's order (rssi descending, ties by the smaller node
 * index), and rssi[j] that link's rssi; roots and unreached nodes have parent -1 and the NaN 0x7FF8000000000000.  children[p] is
 * the number of nodes whose parent is p.  Totals: reached the nodes with hop >= 0, max_hop the largest hop (-1 without a valid
 * root), roots the distinct valid roots, reserved 0.  Roots may repeat; n_roots = 0 is RM_OK with nothing reached.
 * The answer does not depend on the walk, the launch geometry or the table's sort state, and a query changes nothing: no result
 * slot, not the on-air window, not the generator, none of the tables of E11-E15, not the source-candidate cache, not the
 * neighbour query's scratch.  parent is by construction a valid K = 1 table of rm_linkstats_watch_device. */
/* the outputs, [n_nodes] each, by node index: hop is required, the others may be NULL */
typedef struct rm_hops_out { int32_t *hop; int32_t *parent; double *rssi; int32_t *children; } rm_hops_out;
typedef struct rm_hops_totals { int32_t reached; int32_t max_hop; int32_t roots; int32_t reserved; } rm_hops_totals;
/* dev_roots and the arrays dev_out (a host struct) points to are device memory; a root entry outside 0 .. n_nodes - 1 is ignored.
 * The call waits on the context's stream once per level and returns when the outputs are complete; totals (host) may be NULL.
 * RM_ERR_STATE, nothing launched: another medium than RM_MODEL_LOGDIST, between rm_tick_begin and rm_tick_flush, a context with a
 * receiver partition, a context made under RM_GRAPH=1.  RM_ERR_INVALID: NULL ctx, dev_out or hop, an unknown direction, a NaN
 * min_rssi_dbm, n_roots < 0, n_roots > 0 with NULL roots. */
int rm_hops_query_device(rm_context *ctx, int32_t direction, double min_rssi_dbm, const int32_t *dev_roots, int32_t n_roots,
                         const rm_hops_out *dev_out, rm_hops_totals *totals);
/* the same with host arrays; a root outside the table is RM_ERR_INVALID before anything is launched */
int rm_hops_query(rm_context *ctx, int32_t direction, double min_rssi_dbm, const int32_t *roots, int32_t n_roots, const rm_hops_out *out,
                  rm_hops_totals *totals);
/* want[i] = parent[src[i]] for 0 <= src[i] < n_nodes, else -1 (all device memory, n entries; dev_parent [n_nodes] as the query
 * wrote it): enqueued on the context's stream without waiting.  Over source rows of cap entries per slot, dev_want has the shape
 * rm_unicast_query_device takes.  RM_ERR_INVALID: NULL ctx, n < 0, n > 0 with a NULL array. */
int rm_hops_next_device(rm_context *ctx, const int32_t *dev_parent, const int32_t *dev_src, int32_t n, int32_t *dev_want);
/* The same rule over an explicit list of candidate links, a pure host function without a device: entry i says that far[i] may be
 * node[i]'s parent with rssi[i] (NaN rssi entries and entries with node == far are no links).  RM_ERR_INVALID: a NULL out or hop,
 * negative counts, NULL lists with a positive count, a NaN min_rssi_dbm, an index (node, far, root) outside 0 .. n_nodes - 1. */
int rm_hops_from_links(int32_t n_nodes, int32_t n_links, const int32_t *node, const int32_t *far, const double *rssi, double min_rssi_dbm,
                       const int32_t *roots, int32_t n_roots, const rm_hops_out *out, rm_hops_totals *totals);

/* ---- route query: minimum-ETX routes toward a set of roots -------------------------------------------------------------
 * (not reference behaviour.)  A pure function of the node table, the model and the query's
 * parameters, on RM_MODEL_LOGDIST only (with or without RM_LD_SINR); the context's frame error model plays no part.  Per node: the
 * least path cost toward any root over the potential links, each link costing its expected transmission count in units of 1/128,
 * and the parent on such a path.
 * link(j, p, dir) is the hop query's, rssi >= min_rssi_dbm included.  Its cost, one rounding per operation and no fma:
 * snr = rssi - 10.0 * det_log10(ld_noise_lin) (what the SINR medium reports as sinr for a heard link with nothing else on the air);
 * psr = 1.0 for RM_EM_NONE, else rm_error_model_psr's value for (kind, us_per_bit) at (snr, air_us); q = 128.0 / psr,
 * c = floor(q + 0.5).  The link counts iff psr > 0.0 and c <= (double)max_link_cost (a NaN fails both); its cost is (uint32_t)c, which
 * lies in 128 .. max_link_cost.
 * cost[r] = 0 for every root r, whatever its radio state; otherwise cost[j] is the minimum over the counting links of
 * cost[p] + c(j, p) (the least fixed point); a node never reached has RM_ROUTE_UNREACHED.  parent[j] is, among all p with a
 * counting link and cost[p] + c(j, p) == cost[j], the first in the neighbour query's order (rssi descending, then the smaller
 * node index); rssi[j] is that link's rssi, link_cost[j] its c; children[p] is the number of nodes whose parent is p.  Roots and
 * unreached nodes have parent -1, the NaN 0x7FF8000000000000 and link_cost 0.  Totals: reached the nodes with a cost, roots the
 * distinct valid roots, max_cost the largest cost (0 when nothing is reached).  Roots may repeat; n_roots = 0 is RM_OK.
 * With RM_EM_NONE every counting link costs 128: cost = 128 * hop, and parent, rssi and children are the hop query's.
 * The answer does not depend on the walk, the launch geometry, the order of the relaxations or the table's sort state, and a query
 * changes nothing the hop query leaves alone, nor the hop query's scratch.  parent is a valid input of rm_hops_next_device and a
 * valid K = 1 table of rm_linkstats_watch_device. */
#define RM_ROUTE_UNREACHED UINT64_MAX
typedef struct rm_routes_params {
    int32_t direction;      /* RM_NB_HEARD_BY / RM_NB_HEARS: the link between a node and its parent, seen from the node */
    int32_t kind;           /* RM_EM_NONE or RM_EM_OQPSK_250K */
    double us_per_bit;      /* finite and > 0 */
    int64_t air_us;         /* >= 0: the air time of the frame the cost is for */
    double min_rssi_dbm;    /* not a NaN */
    uint32_t max_link_cost; /* 128 .. 65535: a link whose cost is above it does not count */
    uint32_t reserved;      /* 0 */
} rm_routes_params;
/* the outputs, [n_nodes] each, by node index: cost is required, the others may be NULL */
typedef struct rm_routes_out { uint64_t *cost; int32_t *parent; double *rssi; uint32_t *link_cost; int32_t *children; } rm_routes_out;
typedef struct rm_routes_totals { int32_t reached; int32_t roots; uint64_t max_cost; } rm_routes_totals;
/* dev_roots and the arrays dev_out (a host struct) points to are device memory; a root entry outside 0 .. n_nodes - 1 is ignored.
 * The call waits on the context's stream once per round and returns when the outputs are complete; totals (host) may be NULL.
 * RM_ERR_STATE, nothing launched: as rm_hops_query_device.  RM_ERR_INVALID: NULL ctx, params, dev_out or cost, an unknown direction
 * or kind, reserved != 0, us_per_bit not finite and > 0, air_us < 0, a NaN min_rssi_dbm, max_link_cost outside 128 .. 65535,
 * n_roots < 0, n_roots > 0 with NULL roots. */
int rm_routes_query_device(rm_context *ctx, const rm_routes_params *params, const int32_t *dev_roots, int32_t n_roots,
                           const rm_routes_out *dev_out, rm_routes_totals *totals);
/* the same with host arrays; a root outside the table is RM_ERR_INVALID before anything is launched */
int rm_routes_query(rm_context *ctx, const rm_routes_params *params, const int32_t *roots, int32_t n_roots, const rm_routes_out *out,
                    rm_routes_totals *totals);
/* what the context's last completed route query did, for measurements: its relaxation rounds (launches) and the frontier entries
 * they walked in all (entries / n_nodes is the re-labelling factor); 0 and 0 before the first query.  Either may be NULL. */
int rm_routes_last_work(rm_context *ctx, int32_t *rounds, uint64_t *entries);
/* The link cost alone, a pure host function without a device: 1 and *cost when a link of this rssi counts under params at a noise
 * floor of noise_dbm (ld_noise_lin = det_pow10(noise_dbm / 10), as the model derives it), else 0 -- rssi below min_rssi_dbm or NaN,
 * psr 0, a cost above the cap, or parameters the query would refuse.  direction is not looked at; cost may be NULL. */
int rm_routes_link_cost(const rm_routes_params *params, double noise_dbm, double rssi, uint32_t *cost);
/* The same rule over an explicit list of candidate links, a pure host function without a device, like rm_hops_from_links: entry i
 * says that far[i] may be node[i]'s parent with rssi[i].  direction is not looked at.  RM_ERR_INVALID: what rm_hops_from_links and
 * the query's parameter check refuse. */
int rm_routes_from_links(int32_t n_nodes, int32_t n_links, const int32_t *node, const int32_t *far, const double *rssi,
                         const rm_routes_params *params, double noise_dbm, const int32_t *roots, int32_t n_roots, const rm_routes_out *out,
                         rm_routes_totals *totals);

/* ---- measured-route query: minimum-ETX routes over watched-link statistics ---------------------------------------------
 * (not reference behaviour.)  What a collection protocol's link estimator and parent selection
 * do with the counters of the watched links: a pure function of a watch table (peer, rm_link_stats), the parameters, the roots and
 * optionally the current parents, in exact integer arithmetic.  The medium plays no part: accepted on every medium.
 * Tables: peer and stats are [n_nodes][K], K = 1, 2, 4 or 8; peer[j][k] outside 0 .. n_nodes - 1 or equal to j is an empty slot; a
 * far end may occur in several slots of a row.  tables == NULL: the context's own E14 tables as they stand on the stream.
 * Entry (j, k) with far end p, H = heard, D = delivered is usable iff max(min_heard, 1) <= H <= 2^40 and D >= 1; its inbound cost
 * is c_in = max(128, (128 * H + (D >> 1)) / D) in 64-bit unsigned arithmetic: the rounded ETX = 1 / PRR of the link p -> j as j
 * measured it, in units of 1/128.
 * RM_ETX_INBOUND: link (j, k) counts iff the entry is usable and c_in <= max_link_cost; c = c_in.
 * RM_ETX_BOTH: with k' the lowest slot of row p whose peer is j, the link counts iff (j, k) counts under INBOUND, k' exists,
 * (p, k') counts under INBOUND and c = (c_in(j, k) * c_in(p, k') + 64) >> 7 <= max_link_cost (ETX = 1 / (d_f * d_r)).
 * cost[r] = 0 for every valid root; otherwise cost[j] is the minimum over j's counting links of cost[p] + c (the least fixed
 * point); a node never reached has RM_ROUTE_UNREACHED.  For a reached node j that is no root: if cur != NULL, q = cur[j] is a
 * node index, some slot k holds q with a counting link, cost[q] < cost[j] and cost[q] + c(j, k) <= cost[j] + hysteresis, then
 * parent[j] = q, and among those slots the one with the least (c, k) gives slot[j] and link_cost[j] (the keep rule); otherwise
 * among the counting links with cost[p] + c == cost[j] the one with the least (c, p, k) gives parent, slot and link_cost.  Roots and
 * unreached nodes have parent -1, slot -1, link_cost 0.  children[p] is the number of nodes whose parent is p.  Every parent has
 * a strictly smaller cost than its child: the parent array is loop-free for every hysteresis.  cur may be the buffer of
 * out->parent.  Totals: reached, roots (distinct valid roots), max_cost (0 when nothing is reached); with "valid" a cur[j] inside
 * the table: kept the reached non-roots with parent == cur[j], switched those with a valid cur[j] != parent, lost the unreached
 * nodes with a valid cur[j]; all three 0 without cur.  A query changes nothing but its outputs and scratch of its own.  parent is a
 * valid argument of rm_fwd_set_next_device, of rm_hops_next_device and of a K = 1 rm_linkstats_watch_device. */
#define RM_ETX_INBOUND 0
#define RM_ETX_BOTH 1
typedef struct rm_etx_tables {
    const int32_t *peer;        /* [n_nodes][K], aligned to 4 K bytes */
    const rm_link_stats *stats; /* [n_nodes][K], aligned to 8 bytes */
    int32_t K;                  /* 1, 2, 4 or 8 */
    int32_t reserved;           /* 0 */
} rm_etx_tables;
typedef struct rm_etx_params {
    int32_t mode;           /* RM_ETX_INBOUND / RM_ETX_BOTH */
    int32_t reserved;       /* 0 */
    uint32_t min_heard;     /* 0 .. 2^31: an entry with fewer heard frames is not usable */
    uint32_t max_link_cost; /* 128 .. 65535: a link whose cost is above it does not count */
    uint32_t hysteresis;    /* 0 .. 65535, in units of 1/128: how much worse than the least cost the current parent's path may be */
    uint32_t reserved2;     /* 0 */
} rm_etx_params;            /* 24 bytes */
/* the outputs, [n_nodes] each, by node index: cost is required, the others may be NULL */
typedef struct rm_etx_out { uint64_t *cost; int32_t *parent; int32_t *slot; uint32_t *link_cost; int32_t *children; } rm_etx_out;
typedef struct rm_etx_totals { int32_t reached, roots, kept, switched, lost, reserved; uint64_t max_cost; } rm_etx_totals;
/* RM_ETX_INBOUND, min_heard 4, max_link_cost 2048, hysteresis 192 */
void rm_etx_defaults(rm_etx_params *params);
/* RM_OK or RM_ERR_INVALID (NULL, an unknown mode, a field outside its range, a reserved field that is not 0) */
int rm_etx_validate(const rm_etx_params *params);
/* tables (a host struct, or NULL), dev_roots, dev_cur (or NULL) and the arrays dev_out (a host struct) points to are device
 * memory; a root entry outside 0 .. n_nodes - 1 is ignored.  The call waits on the context's stream once per round and returns
 * when the outputs are complete; totals (host) may be NULL.  Nothing is validated on the device: any table content is defined.
 * RM_ERR_STATE, nothing launched: NULL tables while E14 is off or on a context with a receiver partition, between rm_tick_begin
 * and rm_tick_flush, a context made under RM_GRAPH=1.  RM_ERR_INVALID: NULL ctx, params, dev_out or cost, what rm_etx_validate
 * refuses, explicit tables with K outside {1, 2, 4, 8}, reserved != 0, a NULL or misaligned peer or stats, n_roots < 0, n_roots > 0
 * with NULL roots.  A context without nodes: RM_OK with empty totals.
 * Cost: one launch and one wait on the stream per round, and the rounds are at least the tree's depth in links.  On a shallow
 * graph (a field: hundreds of rounds at a million nodes) that is several times faster than reading the table to the host; on a
 * graph tens of thousands of links deep (a line, a band) it is 12 to 64 times SLOWER than rm_etx_from_tables over the same
 * table: a caller with such a table copies it out and calls that. */
int rm_etx_query_device(rm_context *ctx, const rm_etx_params *params, const rm_etx_tables *tables, const int32_t *dev_roots, int32_t n_roots,
                        const int32_t *dev_cur, const rm_etx_out *dev_out, rm_etx_totals *totals);
/* the same with host arrays (explicit tables are host arrays of any alignment); a root outside the table is RM_ERR_INVALID before
 * anything is launched */
int rm_etx_query(rm_context *ctx, const rm_etx_params *params, const rm_etx_tables *tables, const int32_t *roots, int32_t n_roots,
                 const int32_t *cur, const rm_etx_out *out, rm_etx_totals *totals);
/* what the context's last completed measured-route query did, for measurements: its relaxation rounds (launches) and the nodes
 * they examined in all; 0 and 0 before the first query.  Either may be NULL.  Both may vary from run to run; the answer may not. */
int rm_etx_last_work(rm_context *ctx, int32_t *rounds, uint64_t *examined);
/* INBOUND's rule for one entry, a pure host function without a device: 1 and *cost when an entry with these counters counts under
 * params, else 0 -- not usable, a cost above the cap, or parameters rm_etx_validate refuses.  mode is not looked at; cost may be
 * NULL. */
int rm_etx_link_cost(const rm_etx_params *params, uint64_t heard, uint64_t delivered, uint32_t *cost);
/* BOTH's product of two inbound costs, (c_in * c_rev + 64) >> 7 in 64-bit arithmetic, a pure host function */
uint64_t rm_etx_combine(uint32_t c_in, uint32_t c_rev);
/* The same rule on the host by a heap Dijkstra, a pure host function without a device: tables (required), roots, cur (or NULL) and
 * out are host arrays.  RM_ERR_INVALID: what the query's argument checks refuse (alignment aside), n_nodes < 0, a root outside the
 * table. */
int rm_etx_from_tables(int32_t n_nodes, const rm_etx_tables *tables, const rm_etx_params *params, const int32_t *roots, int32_t n_roots,
                       const int32_t *cur, const rm_etx_out *out, rm_etx_totals *totals);

/* ---- forwarding queues: multi-hop packet relay on the device ------------------------------------------------------------------
 * (not reference behaviour.)  Per-node packet queues in device memory and the calls that move
 * packets along a next-hop table from one evaluated tick to the next.  No evaluating call changes: every call here reads a FINISHED
 * result, as the unicast query does, or only the feature's own tables.  Off by default; then nothing is allocated or launched.
 * Memory when on: n_nodes * (24 * queue_slots + 164) bytes -- per node a 128-byte row, the packets, 12 bytes of scratch and one
 * 24-byte record per packet number of an advance or inject list (sized for n_nodes entries at enable; a longer list grows it).  All integers are exact, and no state depends on launch
 * geometry or on the order in which atomics land.
 *
 * State per node j: next[j] (>= 0 a next hop, RM_FWD_NO_ROUTE: every node's value after enable, RM_FWD_SINK), up to queue_slots
 * packets {origin, hops, birth_us, enq_us}, tries, ready_us (both 0 at first) and the counters of rm_fwd_node.  Queue order is
 * ascending (enq_us, birth_us, origin, hops); the head is the first packet in it; slot positions are not observable through the
 * host calls.  j is SENDABLE AT t iff its queue is not empty, ready_us <= t and head.enq_us <= t.  A non-empty queue implies
 * next[j] >= 0.
 *
 * rm_fwd_set_next*: next[j] = parent[j]; an entry outside 0 .. n_nodes - 1 or equal to j becomes -1; then every valid entry of the
 * roots list becomes RM_FWD_SINK -- the parent array and the root list of a hop or route query go in as they lie in device memory.
 * Then the queues are settled: at a node whose next is now SINK every queued packet arrives at time_us (latency time_us - birth_us,
 * hops unchanged); at a node whose next is now -1 every queued packet is dropped as dropped_no_route; tries = 0 at both kinds.
 *
 * rm_fwd_inject*: an entry that is negative or outside the table is padding; every other occurrence of node j generates a packet:
 * next[j] SINK: it arrives at once with 0 hops and latency 0; -1: dropped_no_route; queue full: dropped_full; else
 * {j, 0, time_us, time_us} is pushed.  Duplicates are packets of their own.  A row of rm_traffic_generate_device with n = cap is a
 * valid argument.
 *
 * rm_fwd_sources*: the nodes sendable at time_us in ascending node index, padded with -1 up to cap; *count is the true number,
 * and with count > cap the list holds the first cap.  A ready dev_src of rm_tick_run_sources_device, of the gated tick and of a
 * batch row.  enabled, txprob and channel play no part.
 *
 * The device forms are enqueued on the context's stream and not waited for; the scratch is sized at enable for lists of up to
 * n_nodes entries, and only an inject or candidate list longer than that makes its call wait for the stream once, to grow it.
 * rm_fwd_enable on a context without nodes is RM_ERR_STATE.
 * rm_fwd_advance*: enqueued on the context's stream, not waited for.  Reads result slot `slot` of the last evaluating call under the
 * unicast query's state rules (slot 0 is also the last lone tick).  A slot that overflowed its link capacity or was dropped
 * (RM_UC_LOST's condition): nothing changes but skipped_slots++.  Otherwise, for packet numbers p = 0 .. P - 1 -- with a candidate
 * list P = min(n_cand, n_new) and the candidate j is cand[p] (the list handed to the evaluating call: a gated tick keeps packet
 * numbers in their places); with dev_cand NULL P = n_new and j = recs[p].src -- and t_end = recs[p].start_us + recs[p].air_us:
 *  1. j outside the table: nothing.  2. j also at a lower p of this slot: stray++.  3. j not sendable at recs[p].start_us, judged on
 *  the state at the start of the call: stray++.  4. otherwise j PARTICIPATES: attempts[j]++, w = next[j], and the attempt is
 *  deferred if recs[p].src != j; failed if the unicast status of (slot, p, w) is not RM_UC_DELIVERED; acked if it is and w is a sink
 *  or w ACCEPTS; failed and rejected[w]++ if it is and w rejects.  5. With A[w] the participants of this call whose frame was
 *  delivered at w, a relay w accepts iff len_start[w] + A[w] <= queue_slots (len_start: at the start of the call): all of them or
 *  none; w's own pop in the same call does not make room.  6. acked: j's head (the head at the start of the call) is popped,
 *  tries = 0, ready_us = t_end, acked[j]++; at a sink the packet's origin o gets arrived[o]++, latency_us_sum[o] += t_end - birth_us,
 *  latency_us_max[o] raised to it, hops_sum[o] += hops + 1; else if hops + 1 > max_hops it is dropped as dropped_ttl AT w; else
 *  {origin, hops + 1, birth_us, t_end} is pushed at w and queue_max[w] is raised to len_start[w] + the packets pushed at w in this
 *  call.  7. failed / deferred: failed[j]++ or deferred[j]++, tries++; if tries > max_retries the head is popped as dropped_retries,
 *  tries = 0, ready_us = t_end; else ready_us = t_end + r * backoff_unit_us with BE = min(min_be + tries - 1, max_be), r = 0 for
 *  BE = 0, else h2 >> (64 - BE), h1 = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (uint64_t)(uint32_t)j) ^ (uint64_t)start_us),
 *  h2 = mix64(h1 ^ (uint64_t)tries) (mix64: the hash of the link draws).
 * Every drop also does lost[origin]++ and dropped[node where it was dropped]++.  A batch: one advance per slot, ascending.
 * Identities: generated = arrived + the four dropped_* + in_flight; attempts = acked + failed + deferred per node.
 *
 * RM_ERR_STATE, nothing launched: the feature is off; for advance what rm_unicast_query refuses (no evaluated result, a receiver
 * partition, a gathered / rm_dist_* / rm_group_* form, RM_GRAPH=1); rm_fwd_enable on a context made under RM_GRAPH=1.
 * RM_ERR_INVALID, nothing launched: bad parameters, NULL arguments, negative counts or times, cap < 1, slot outside the last call's
 * slots, a host roots / inject entry >= n_nodes.  rm_node_update, rm_nodes_move, rm_set_model and rm_nodes_upload with the same
 * node count keep everything; rm_nodes_upload with another node count switches the feature off. */
#define RM_FWD_NO_ROUTE (-1)
#define RM_FWD_SINK (-2)
typedef struct rm_fwd_params {
    int32_t queue_slots;     /* 1, 2, 4, 8 or 16 */
    int32_t max_retries;     /* 0 .. 15 */
    int32_t min_be, max_be;  /* 0 <= min_be <= max_be <= 8 */
    int32_t max_hops;        /* 1 .. 255 */
    int32_t reserved;        /* 0 */
    int64_t backoff_unit_us; /* 0 .. 2^32 */
    uint64_t seed;
} rm_fwd_params; /* 40 bytes */
typedef struct rm_fwd_packet { int32_t origin; int32_t hops; int64_t birth_us; int64_t enq_us; } rm_fwd_packet; /* 24 bytes */
typedef struct rm_fwd_node { /* 128 bytes: the table's row */
    uint64_t generated, arrived, lost, latency_us_sum, latency_us_max, hops_sum;  /* as origin */
    uint64_t attempts, acked, failed, deferred, rejected, dropped;               /* as relay */
    int64_t ready_us;
    int32_t next, queue_len, queue_max, tries;
    uint32_t slot_mask;  /* the device table only (rm_fwd_read gives 0): bit s set = slot s of the node's packets is occupied */
    uint32_t reserved;
} rm_fwd_node;
typedef struct rm_fwd_totals {
    uint64_t generated, arrived, dropped_retries, dropped_no_route, dropped_full, dropped_ttl, in_flight, stray, skipped_slots,
        latency_us_sum, hops_sum;
} rm_fwd_totals; /* 88 bytes */
void rm_fwd_defaults(rm_fwd_params *p); /* 8 slots, 3 retries, BE 3 .. 5, 64 hops, 320 us, seed 0 */
/* pure host functions, no device: RM_OK or RM_ERR_INVALID; *delay_us = r * backoff_unit_us for tries >= 1, node >= 0, start_us >= 0 */
int rm_fwd_validate(const rm_fwd_params *p);
int rm_fwd_backoff(const rm_fwd_params *p, int32_t node, int64_t start_us, int32_t tries, int64_t *delay_us);
/* enable (again: with new parameters, everything cleared, next -1 everywhere), release, state */
int rm_fwd_enable(rm_context *ctx, const rm_fwd_params *p);
int rm_fwd_disable(rm_context *ctx);
int rm_fwd_enabled(const rm_context *ctx);
int rm_fwd_get_params(const rm_context *ctx, rm_fwd_params *out); /* the enabled parameters: queue_slots sizes rm_fwd_queue_read's out */
/* clears counters, totals and queues (tries, ready_us 0); keeps next and the parameters */
int rm_fwd_reset(rm_context *ctx);
int rm_fwd_set_next_device(rm_context *ctx, const int32_t *dev_parent /* [n_nodes] */, const int32_t *dev_roots, int32_t n_roots, int64_t time_us);
int rm_fwd_set_next(rm_context *ctx, const int32_t *parent /* [n_nodes] */, const int32_t *roots, int32_t n_roots, int64_t time_us);
int rm_fwd_inject_device(rm_context *ctx, const int32_t *dev_src, int32_t n, int64_t time_us);
int rm_fwd_inject(rm_context *ctx, const int32_t *src, int32_t n, int64_t time_us);
int rm_fwd_sources_device(rm_context *ctx, int64_t time_us, int32_t cap, int32_t *dev_src /* [cap] */, int32_t *dev_count);
int rm_fwd_sources(rm_context *ctx, int64_t time_us, int32_t cap, int32_t *src /* [cap] */, int32_t *count); /* synchronises */
int rm_fwd_advance_device(rm_context *ctx, int32_t slot, const int32_t *dev_cand /* or NULL */, int32_t n_cand);
int rm_fwd_advance(rm_context *ctx, int32_t slot, const int32_t *cand /* or NULL */, int32_t n_cand); /* uploads the list */
/* n rows (nodes NULL: all, n = n_nodes) and the totals (may be NULL; out may be NULL with n = 0); synchronises */
int rm_fwd_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_fwd_node *out, rm_fwd_totals *totals);
/* the listed nodes' packets in queue order, queue_slots entries per node (unused ones zeroed), and their number; synchronises */
int rm_fwd_queue_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_fwd_packet *out /* [n][queue_slots] */, int32_t *len /* [n] */);
/* the tables in device memory (valid until disable, another enable or another node count); any pointer may be NULL */
int rm_fwd_device(rm_context *ctx, const rm_fwd_node **dev_node, const rm_fwd_packet **dev_packets /* [n_nodes][queue_slots] */,
                  const rm_fwd_totals **dev_totals);

/* ---- dissemination floods: Trickle-timed broadcast relay on the device ---------------------------------------------------------
 * (not reference behaviour.)  One-to-all dissemination under Trickle's suppression rule
 * (RFC 6206, one data version): per-node flood state in device memory and the calls that move it from one evaluated tick to the
 * next.  No evaluating call changes: every call here reads a FINISHED result, as the unicast query does, or only the feature's own
 * table.  Off by default; then nothing is allocated or launched.  Memory when on: n_nodes * 84 bytes (a 64-byte row, 16 bytes of
 * scratch, one word per packet number of an advance or seed list, sized for n_nodes entries at enable; a longer list grows it).
 * All integers are exact, and no state depends on launch geometry or on the order in which atomics land.
 *
 * State per node j (rm_flood_node): first_us (-1: j does not have the data), start_us and fire_us of its running interval (-1:
 * nothing scheduled), rssi_bits (the bits of the first link's rssi, 0 at a seed), parent (-1 at a seed and without the data),
 * hop (-1 without the data), interval m, c, and the counters sent, suppressed, heard, deferred.
 * Schedule: a node that got the data at first_us has intervals of length I_m = imin_us << min(m, doublings) that start at
 * s_m = first_us + sum of I_i over i < m; it fires at f_m = s_m + I_m / 2 + r, r = (h * (I_m / 2)) >> 64 (the 128-bit product),
 * h = mix64(mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (uint64_t)(uint32_t)j) ^ (uint64_t)first_us) ^ (uint64_t)m) (mix64: the
 * hash of the link draws).  With m == max_intervals the node is done: start_us = fire_us = -1.  j is DUE AT t iff it has the
 * data, m < max_intervals and fire_us <= t.  rm_flood_fire is this rule as a pure host function.
 *
 * rm_flood_seed*: a valid entry that does not have the data gets first_us = time_us, hop 0, parent -1, m 0, c 0 and its schedule
 * (seeds++, covered++); entries outside the table and nodes that have the data, duplicates included, change nothing.
 *
 * rm_flood_sources*: one walk over the nodes.  A node due at time_us with redundancy k > 0 and c >= k is SUPPRESSED: suppressed++,
 * m++, c = 0, the next schedule; nothing else happens to it in this call, even if the new fire_us <= time_us.  Every other due
 * node is listed in ascending node index, padded with -1 up to cap; *count is the true number, and with count > cap the list
 * holds the first cap.  A listed node's state does not change: it stays due until an advance sees it transmit.  A ready dev_src
 * of rm_tick_run_sources_device, of the gated tick and of a batch row.
 *
 * rm_flood_advance*: slot, state rules and candidate list as rm_fwd_advance*.  A slot that overflowed its link capacity or was
 * dropped: nothing changes but skipped_slots++.  All judgments are on the state at the start of the call.
 *  Transmitters, packet numbers p = 0 .. P - 1 with candidate j: j outside the table or without the data: nothing (foreign
 *  traffic); a later occurrence of j: stray++; j not due at recs[p].start_us: stray++; recs[p].src != j (a gate deferred it):
 *  deferred[j]++ and j stays due; otherwise j SENT: sent[j]++, m++, c = 0, the next schedule.
 *  Receivers, every link of the slot with verdict RM_DELIVERED, of packet p (any p < n_new) to node d in the table, whose
 *  s = recs[p].src is in the table and has the data, t_end = recs[p].start_us + recs[p].air_us: heard[d]++.  If d has the data,
 *  does not send in this call and t_end >= start_us[d]: c[d]++.  If d does not have the data and hop[s] + 1 <= max_hops: among
 *  all such links of this slot at d the one with the least (t_end, p) wins and d gets first_us = t_end, parent = s,
 *  hop = hop[s] + 1, rssi_bits, m = 0, c = 0 and its schedule (covered++); the other copies count in heard only.
 * Identities: covered = seeds + first receptions = the nodes with first_us >= 0; the sums of the per-node sent / suppressed /
 * heard / deferred are the totals; interval = sent + suppressed per node.  max_hop and last_first_us are the maxima over the
 * covered nodes (0 when there is none).
 *
 * rm_flood_tree_device gathers parent (and hop, unless NULL) into contiguous arrays: dev_parent is a valid argument of
 * rm_fwd_set_next_device (with the seed list as roots), of rm_hops_next_device and of a K = 1 rm_linkstats_watch_device.
 *
 * The device forms are enqueued on the context's stream and not waited for.  RM_ERR_STATE, nothing launched: the feature is off;
 * for advance what rm_unicast_query refuses (no evaluated result, a receiver partition, a gathered / rm_dist_* / rm_group_* form,
 * RM_GRAPH=1); rm_flood_enable on a context made under RM_GRAPH=1 or without nodes.  RM_ERR_INVALID, nothing launched: bad
 * parameters, NULL arguments, negative counts or times, cap < 1, slot outside the last call's slots, a host list entry >= n_nodes.
 * rm_nodes_upload with another node count switches the feature off; the same count, rm_node_update, rm_nodes_move and
 * rm_set_model keep everything.  Out of scope: several data versions and Trickle's inconsistency reset, payload lengths,
 * partitions and the multi-rank forms. */
typedef struct rm_flood_params {
    int64_t imin_us;       /* 2 .. 2^32 */
    int32_t doublings;     /* 0 .. 16 */
    int32_t max_intervals; /* 1 .. 64 */
    int32_t redundancy;    /* 0 .. 255; 0: never suppress */
    int32_t max_hops;      /* 1 .. 65535 */
    uint64_t seed;
} rm_flood_params; /* 32 bytes */
typedef struct rm_flood_node { /* 64 bytes: the table's row */
    int64_t first_us, start_us, fire_us;
    uint64_t rssi_bits;
    int32_t parent, hop, interval, c;
    uint32_t sent, suppressed, heard, deferred;
} rm_flood_node;
typedef struct rm_flood_totals {
    uint64_t covered, seeds, sent, suppressed, heard, deferred, stray, skipped_slots, max_hop, last_first_us;
} rm_flood_totals; /* 80 bytes */
void rm_flood_defaults(rm_flood_params *p); /* 8000 us, 4 doublings, 8 intervals, k = 2, 255 hops, seed 0 */
/* pure host functions, no device: RM_OK or RM_ERR_INVALID; node >= 0, first_us >= 0, 0 <= m <= max_intervals */
int rm_flood_validate(const rm_flood_params *p);
int rm_flood_fire(const rm_flood_params *p, int32_t node, int64_t first_us, int32_t m, int64_t *start_us, int64_t *fire_us);
/* enable (again: with new parameters, everything cleared), release, state */
int rm_flood_enable(rm_context *ctx, const rm_flood_params *p);
int rm_flood_disable(rm_context *ctx);
int rm_flood_enabled(const rm_context *ctx);
int rm_flood_get_params(const rm_context *ctx, rm_flood_params *out);
int rm_flood_reset(rm_context *ctx); /* nobody has the data, counters and totals zero; keeps the parameters */
int rm_flood_seed_device(rm_context *ctx, const int32_t *dev_nodes, int32_t n, int64_t time_us);
int rm_flood_seed(rm_context *ctx, const int32_t *nodes, int32_t n, int64_t time_us);
int rm_flood_sources_device(rm_context *ctx, int64_t time_us, int32_t cap, int32_t *dev_src /* [cap] */, int32_t *dev_count);
int rm_flood_sources(rm_context *ctx, int64_t time_us, int32_t cap, int32_t *src /* [cap] */, int32_t *count); /* synchronises */
int rm_flood_advance_device(rm_context *ctx, int32_t slot, const int32_t *dev_cand /* or NULL */, int32_t n_cand);
int rm_flood_advance(rm_context *ctx, int32_t slot, const int32_t *cand /* or NULL */, int32_t n_cand); /* uploads the list */
/* n rows (nodes NULL: all, n = n_nodes) and the totals (may be NULL; out may be NULL with n = 0); synchronises */
int rm_flood_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_flood_node *out, rm_flood_totals *totals);
/* the table in device memory (valid until disable, another enable or another node count); either pointer may be NULL */
int rm_flood_device(rm_context *ctx, const rm_flood_node **dev_node, const rm_flood_totals **dev_totals);
/* the measured tree: parent and hop by node index, int32[n_nodes] each, in device memory (dev_hop may be NULL); not waited for */
int rm_flood_tree_device(rm_context *ctx, int32_t *dev_parent, int32_t *dev_hop);

/* ---- neighbour tables: discover, evict and expire watched peers on the device ----------------------------------------------------
 * (not reference behaviour.)  What a link estimator's neighbour table does -- learn peers
 * from the frames heard, keep a small table, throw out the dead and the bad, protect the parent -- on the watched-link
 * statistics' two tables (peer and rm_link_stats, [n_nodes][K]), by an order-independent rule: at most one admission per receiver
 * per finished slot, the admitted sender chosen by a maximum, the slot to fill or evict chosen from the tables as they stood at the
 * start of the call.  No evaluating call changes and the watched links' pass does not change: every call here reads a FINISHED
 * result, as the unicast query does, or only the tables.  Off by default; then nothing is allocated or launched.  Memory when on:
 * n_nodes * 40 bytes (a 32-byte row of counters, one 64-bit word of scratch that is 0 between calls) and the host forms' staging.
 *
 * Judgments, all on peer and stats as they stand on the stream at the start of the call, for a node d and its slot k:
 *  EMPTY   peer[d][k] is outside 0 .. n_nodes-1 or equals d.
 *  PINNED  a pin array was given, pin[d] is in 0 .. n_nodes-1 and peer[d][k] == pin[d].  The parent arrays of the hop, route and
 *          measured-route queries and of rm_flood_tree_device go in as they lie in device memory.
 *  STALE AT t  timeout_us > 0 and (last_start_us == INT64_MIN, or t >= timeout_us and last_start_us < t - timeout_us): a watched
 *          entry that never heard anything is stale.
 *  POOR    evict_cost > 0, heard >= max(min_heard, 1) and (delivered == 0 or c_in > evict_cost), with
 *          c_in = max(128, (128 * heard + (delivered >> 1)) / delivered) in uint64: the measured-route query's entry cost.
 *
 * rm_nbtable_update*: slot and state rules as rm_flood_advance*.  A slot that overflowed its link capacity or was dropped: nothing
 * changes but skipped_slots++.  Any other slot: updates++, then
 *  (1) BIDS.  Link i of the slot, of packet p, s = recs[p].src, d = dst[i], bids iff s and d are node indices, s != d, no slot of
 *      row d holds s, rssi[i] >= admit_rssi_dbm (NaN fails) and, with require_delivered, the link's final verdict is RM_DELIVERED.
 *      Its key is (qc, -s), qc = rm_linkstats_q8(rssi[i]) clamped to -2^30 .. 2^30: the greatest qc wins, ties go to the least s.
 *  (2) SETTLE.  A node d with a winning bid s takes the first that applies: (a) its lowest empty slot; (b) among the slots that are
 *      not pinned and stale at time_us the least (last_start_us, k): evicted_stale[d]++; (c) among the slots that are not pinned
 *      and poor those with delivered == 0 first (the least k of them), then the greatest c_in, then the least k:
 *      evicted_poor[d]++; (d) refused[d]++ and nothing changes.  In (a) to (c) peer[d][k] = s, the entry is cleared and
 *      admitted[d]++.
 *  (3) COUNT.  Every link of the slot from an admitted s to its d -- duplicates, undelivered and weak copies included -- is added
 *      to the fresh entry exactly as the watched links' pass adds a link.  ticks_counted / ticks_skipped are not touched.
 * A row's valid entries stay distinct.  The answer is a pure function of (the tables at the start, the slot's result, the
 * parameters, time_us, pin): nothing depends on launch geometry or on the order in which atomics land.
 * The watched links' pass counts a whole batch before the first update of its slots can run: a peer admitted from slot b of a
 * batch is not counted in slots b+1 .. of that batch, and is when the ticks run one by one with an update after each.  Both orders
 * are deterministic and equal rm_nbtable_from_result applied in the same order.
 *
 * rm_nbtable_expire*: one walk over the table; every slot that is not empty, not pinned and stale at time_us becomes empty (peer
 * -1, the entry cleared, expired[d]++).  Poor slots are left alone.  No result slot is read.
 *
 * Identities: the per-node sums are the totals; per node and in total admitted >= evicted_stale + evicted_poor.
 * The device forms are enqueued on the context's stream and not waited for; the host forms upload the pin array first.
 * RM_ERR_INVALID, nothing launched: bad parameters or a non-zero reserved field, NULL ctx or params, negative time_us, slot outside
 * the last call's slots, a host pin entry >= n_nodes (negative host entries: no pin; device entries outside the table pin
 * nothing).  RM_ERR_STATE, nothing launched: the feature off, the watched-link statistics off, for update what rm_unicast_query
 * refuses (no evaluated result, a receiver partition, a gathered / rm_dist_* / rm_group_* form), rm_nbtable_enable on a context
 * made under RM_GRAPH=1 or without nodes.  Arguments are checked before state.
 * rm_linkstats_enable with the same K keeps everything; K = 0, another K or rm_nodes_upload with another node count switch this
 * feature off with the statistics.  rm_linkstats_reset makes every entry stale.  rm_linkstats_watch* stays allowed.  Out of
 * scope: replacing a healthy neighbour, several admissions per node and slot, smoothing, blacklists, K > 8, partitions. */
typedef struct rm_nbtable_params {
    double admit_rssi_dbm;     /* finite; a link below it never bids */
    int64_t timeout_us;        /* 0 .. 2^62; 0: no slot is ever stale */
    uint32_t min_heard;        /* 0 .. 2^31 */
    uint32_t evict_cost;       /* 0, or 128 .. 2^32-1, in units of 1/128; 0: no slot is ever poor */
    int32_t require_delivered; /* 0 or 1 */
    int32_t reserved;          /* 0 */
} rm_nbtable_params; /* 32 bytes */
typedef struct rm_nbtable_node { /* 32 bytes: the table's row */
    uint32_t admitted, evicted_stale, evicted_poor, refused, expired, reserved[3];
} rm_nbtable_node;
typedef struct rm_nbtable_totals {
    uint64_t updates, skipped_slots, admitted, evicted_stale, evicted_poor, refused, expired, reserved;
} rm_nbtable_totals; /* 64 bytes */
void rm_nbtable_defaults(rm_nbtable_params *p); /* -95.0 dBm, 60 000 000 us, min_heard 4, evict_cost 1024, require_delivered 1 */
/* pure host function, no device: RM_OK or RM_ERR_INVALID */
int rm_nbtable_validate(const rm_nbtable_params *p);
/* enable (again: new parameters, counters and totals zero; the statistics' tables are never touched here), release, state */
int rm_nbtable_enable(rm_context *ctx, const rm_nbtable_params *p);
int rm_nbtable_disable(rm_context *ctx);
int rm_nbtable_enabled(const rm_context *ctx);
int rm_nbtable_get_params(const rm_context *ctx, rm_nbtable_params *out);
int rm_nbtable_reset(rm_context *ctx); /* counters and totals zero; the statistics' tables are left alone */
int rm_nbtable_update_device(rm_context *ctx, int32_t slot, int64_t time_us, const int32_t *dev_pin /* [n_nodes] or NULL */);
int rm_nbtable_update(rm_context *ctx, int32_t slot, int64_t time_us, const int32_t *pin /* [n_nodes] or NULL */); /* uploads pin */
int rm_nbtable_expire_device(rm_context *ctx, int64_t time_us, const int32_t *dev_pin /* [n_nodes] or NULL */);
int rm_nbtable_expire(rm_context *ctx, int64_t time_us, const int32_t *pin /* [n_nodes] or NULL */);
/* n rows (nodes NULL: all, n = n_nodes) and the totals (may be NULL; out may be NULL with n = 0); synchronises.  The peers and the
 * entries are read with rm_linkstats_peers_get and rm_linkstats_read. */
int rm_nbtable_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_nbtable_node *out, rm_nbtable_totals *totals);
/* the counters in device memory (valid until disable, another enable, or the statistics going off); either pointer may be NULL */
int rm_nbtable_device(rm_context *ctx, const rm_nbtable_node **dev_node, const rm_nbtable_totals **dev_totals);
/* pure host functions, no device: the update rule over one tick's host result (src[n_packets] and start_us[n_packets] are the
 * packets' sources and starts; reads pkt_offset, dst, verdict, rssi or pkt_rssi, sinr) and the expire walk, on host tables peer
 * and stats [n_nodes][K] in place; node [n_nodes] and totals are ADDED to (either may be NULL).  A host result has no lost flag:
 * capacity problems are the caller's.  RM_ERR_INVALID: NULL arguments, bad parameters, K not 1, 2, 4 or 8, n_nodes < 0, negative
 * time_us, a pin entry >= n_nodes. */
int rm_nbtable_from_result(const rm_host_result *r, const int32_t *src, const int64_t *start_us, int32_t n_nodes, int32_t K, int32_t *peer,
                           rm_link_stats *stats, const rm_nbtable_params *params, int64_t time_us, const int32_t *pin /* or NULL */,
                           rm_nbtable_node *node, rm_nbtable_totals *totals);
int rm_nbtable_expire_tables(int32_t n_nodes, int32_t K, int32_t *peer, rm_link_stats *stats, const rm_nbtable_params *params, int64_t time_us,
                             const int32_t *pin /* or NULL */, rm_nbtable_node *node, rm_nbtable_totals *totals);

/* ---- link estimator: EWMA ETX over counter windows and forwarding acks ----------------------------------------------------------
 * (not reference behaviour.)  What CTP's 4-bit estimator or Contiki's link-stats keep per
 * neighbour: a smoothed ETX in the measured-route query's units of 1/128, fed by windows of the watched links' counters (beacon
 * samples) and by windows of the forwarding queues' acked / failed attempts toward the current next hop (data samples).  The
 * estimator READS a watch table (peer and rm_link_stats, [n_nodes][K]) and optionally a forwarding table (rm_fwd_node [n_nodes])
 * -- the context's own or the caller's -- and never writes them: rm_linkstats_reset is not needed to start a window, so the
 * neighbour tables' stale and poor judgments stay as they are.  It keeps tables of its own: an rm_linkest_entry per (node, slot),
 * an rm_linkest_node per node, the totals, and the PUBLISHED table -- a valid rm_etx_tables (rm_linkest_tables) whose entry with an
 * estimate is {heard = etx, delivered = 128, 0, 0, INT64_MAX, INT64_MIN} and whose entry without one is the cleared entry, with
 * pub_peer == entry.peer.  The measured-route query's c_in of such an entry is exactly etx (128 .. 65535), so rm_etx_query_device
 * over rm_linkest_tables with min_heard <= 128 routes over the smoothed costs.  Off by default; then nothing is allocated or
 * launched.  Memory when on: n_nodes * (K * 84 + 32) bytes.  No evaluating call changes.
 *
 * rm_linkest_fold*: one launch.  inputs == NULL: the context's E14 tables, and E19's rows while E19 is on (else no data step).
 * All judgments are on the inputs as they stand on the stream at the start of the call; the result is a pure function of (the
 * state at the start, the inputs, the parameters) and does not depend on launch geometry or on the order of atomics.  folds++.
 *  ewma(a, old, s) = s when old == 0, else (a * old + (256 - a) * s + 128) >> 8 in 64-bit arithmetic: between min(old, s) and
 *  max(old, s), so within 128 .. max_etx.  The rounding leaves a dead band: under a constant sample s the estimate stops moving
 *  once (256 - a) * (old - s) <= 128 from above, or (256 - a) * (s - old) < 128 from below (up to 4 units at a = 230; none at a = 0).
 *  sample(dn, dd) = max_etx when dd == 0, else min(max_etx, max(128, (128 * dn + (dd >> 1)) / dd)) in uint64 arithmetic modulo
 *  2^64 (exact for dn < 2^57).
 *  BEACON STEP, entry (j, k), p = peer[j][k], H = heard, D = delivered:
 *  (1) p empty (outside 0 .. n_nodes-1, or j): the entry becomes {0, 0, 0, 0, 0, -1}; cleared++ if entry.peer was not -1.
 *  (2) else if p != entry.peer or H < base_heard or D < base_delivered: the entry becomes {0, 0, 0, 0, 0, p}; restarted++ per node
 *      and in total (an admission, an eviction, rm_linkstats_watch, rm_linkstats_reset).
 *  (3) then, kept or restarted: dH = H - base_heard, dD = D - base_delivered; if beacon_window > 0 and dH >= beacon_window:
 *      etx = ewma(beacon_alpha_q8, etx, sample(dH, dD)), windows++, beacon_samples++, base_heard = H, base_delivered = D.
 *  DATA STEP, node j, only with a forwarding table and data_window > 0, after the row's beacon step; w = fwd[j].next,
 *  A = acked, T = acked + failed (deferred attempts were not on the air):
 *  (1) w != base_next or T < base_tx or A < base_ack: base_next = w, base_tx = T, base_ack = A, no sample.
 *  (2) else if w is a node index other than j and T - base_tx >= data_window: dT = T - base_tx, dA = A - base_ack, base_tx = T,
 *      base_ack = A; with k the lowest slot of row j whose entry.peer == w: none: data_unmatched++ per node and in total; else
 *      etx[j][k] = ewma(data_alpha_q8, etx, sample(dT, dA)), data_windows++ of the entry, data_samples++ per node and in total.
 *  estimates is the number of entries with etx != 0.  The published entry is rewritten whenever etx or peer changes.
 * Identities: the per-node restarted / data_samples / data_unmatched sum to the totals; beacon_samples is the sum of windows and
 * data_samples the sum of data_windows over entries that were not cleared or restarted since.
 * The device form is enqueued on the context's stream and not waited for; the host form uploads the inputs first.
 * RM_ERR_INVALID, nothing launched: NULL ctx or params, what rm_linkest_validate refuses, K outside {1, 2, 4, 8}, explicit inputs
 * with another K than the enabled one, a non-zero reserved field, a NULL peer or stats, or (device form) peer not aligned to 4 K
 * bytes, stats or fwd not to 8.  RM_ERR_STATE, nothing launched: the feature off; inputs == NULL while E14 is off or has another
 * K; a context with a receiver partition; between rm_tick_begin and rm_tick_flush; rm_linkest_enable on a context made under
 * RM_GRAPH=1 or without nodes.  Arguments are checked before state.  rm_nodes_upload with another node count switches the feature
 * off; rm_linkstats_enable with another K leaves it on, and own-table folds are RM_ERR_STATE until rm_linkest_enable with that K;
 * rm_node_update, rm_nodes_move, rm_set_model and rm_seed keep everything.  Out of scope: samples over the sender's sent count
 * (E11), the neighbour tables judging by the estimate, estimate-aware hysteresis, K > 8, partitions and the multi-rank forms. */
typedef struct rm_linkest_params {
    uint32_t beacon_window;   /* 0 .. 2^31 heard frames per beacon sample; 0: no beacon samples */
    uint32_t data_window;     /* 0 .. 2^31 acked + failed attempts per data sample; 0: no data samples */
    uint32_t beacon_alpha_q8; /* 0 .. 255: the weight of the OLD estimate out of 256 */
    uint32_t data_alpha_q8;   /* 0 .. 255 */
    uint32_t max_etx;         /* 128 .. 65535, in units of 1/128: a sample's cap, and a window without a delivery */
    uint32_t reserved;        /* 0 */
} rm_linkest_params; /* 24 bytes */
typedef struct rm_linkest_entry {
    uint64_t base_heard, base_delivered; /* the counters at the last sample or restart */
    uint32_t etx;                        /* 0: no estimate yet; else 128 .. max_etx */
    uint32_t windows, data_windows;      /* samples folded into etx since the last restart */
    int32_t peer;                        /* -1: empty */
} rm_linkest_entry; /* 32 bytes */
typedef struct rm_linkest_node {
    uint64_t base_tx, base_ack;
    int32_t base_next; /* -1 after enable */
    uint32_t data_samples, data_unmatched, restarted;
} rm_linkest_node; /* 32 bytes */
typedef struct rm_linkest_totals {
    uint64_t folds, beacon_samples, data_samples, data_unmatched, restarted, cleared, estimates, reserved;
} rm_linkest_totals; /* 64 bytes */
typedef struct rm_linkest_inputs {
    const int32_t *peer;        /* [n_nodes][K] */
    const rm_link_stats *stats; /* [n_nodes][K] */
    const rm_fwd_node *fwd;     /* [n_nodes], or NULL: no data step */
    int32_t K;                  /* the enabled K */
    int32_t reserved;           /* 0 */
} rm_linkest_inputs;
void rm_linkest_defaults(rm_linkest_params *p); /* windows 3 and 5, both alphas 230, max_etx 6400: CTP's windows, 0.9, an ETX of 50 */
/* pure host function, no device: RM_OK or RM_ERR_INVALID */
int rm_linkest_validate(const rm_linkest_params *p);
/* enable (again: new K and parameters, everything in its after-enable state; the old tables are released first, so an enable that
 * fails with RM_ERR_HIP leaves the feature OFF, not as it was), release, state (K, or 0 while off) */
int rm_linkest_enable(rm_context *ctx, int32_t K, const rm_linkest_params *p);
int rm_linkest_disable(rm_context *ctx);
int rm_linkest_enabled(const rm_context *ctx);
int rm_linkest_get_params(const rm_context *ctx, rm_linkest_params *out);
int rm_linkest_reset(rm_context *ctx); /* every table back to its after-enable state; K and the parameters stay */
/* inputs: a host struct (or NULL) whose arrays are device memory; enqueued, not waited for */
int rm_linkest_fold_device(rm_context *ctx, const rm_linkest_inputs *dev_inputs);
/* the same with host arrays of any alignment, uploaded first */
int rm_linkest_fold(rm_context *ctx, const rm_linkest_inputs *inputs);
/* n rows of K entries (entry_out [n][K]) and of node state (node_out [n]), nodes NULL: all, n = n_nodes; any output may be NULL;
 * synchronises */
int rm_linkest_read(rm_context *ctx, const int32_t *nodes, int32_t n, rm_linkest_entry *entry_out, rm_linkest_node *node_out,
                    rm_linkest_totals *totals);
/* the tables in device memory (valid until disable, another enable or another node count); any pointer may be NULL */
int rm_linkest_device(rm_context *ctx, const rm_linkest_entry **dev_entry, const rm_linkest_node **dev_node, const rm_linkest_totals **dev_totals);
/* the published table as the measured-route query's explicit tables (device pointers; the same lifetime) */
int rm_linkest_tables(rm_context *ctx, rm_etx_tables *out);
/* the fold over host arrays in place, a pure host function without a device: entry, pub_peer and pub_stats are [n_nodes][K], node
 * [n_nodes]; totals (may be NULL) is ADDED to.  RM_ERR_INVALID: NULL arguments, bad parameters or inputs, n_nodes < 0. */
int rm_linkest_fold_tables(int32_t n_nodes, const rm_linkest_inputs *inputs, const rm_linkest_params *params, rm_linkest_entry *entry,
                           rm_linkest_node *node, int32_t *pub_peer, rm_link_stats *pub_stats, rm_linkest_totals *totals);

/* ---- several devices behind one caller --------------------------------------------------------------
 * The reference host is ONE process (Main.java:65-73): a group drives n contexts from one host thread, one
 * per device (an ordinal may repeat: several partitions on one GPU).  Receivers are partitioned over the
 * members by region (rm_set_partition_spatial; or by node index range, rm_group_set_partitioning); a tick's
 * Tx records are on the host already, so they are simply handed to every member -- no all-gather; every
 * member evaluates them against its receivers, the launches of all members are enqueued before any result
 * is waited for, and the heard links are merged packet-major / node ascending (a k-way merge by node index).
 * Probabilistic links: the per-packet draw counts (and, for regions, the drawing links' nodes) are exchanged
 * through the host and every member places its draws among the other members' (rm_tick_finish_draws*), so
 * verdicts, Tx-failure flags and the java.util.Random state are those of one context.  Everything else of a member (reception stage, node-info, device-resident results) is reached
 * through rm_group_context. */
typedef struct rm_group rm_group;
int rm_group_create(int32_t n_members, const int32_t *device_ordinals, rm_group **out);
void rm_group_destroy(rm_group *g);
/* members own regions of the plane (default, rm_set_partition_spatial) or ranges of node indices (spatial = 0);
 * before rm_group_nodes_upload */
int rm_group_set_partitioning(rm_group *g, int32_t spatial);
int rm_group_size(const rm_group *g);
rm_context *rm_group_context(rm_group *g, int32_t member);
int rm_group_set_model(rm_group *g, const rm_model_params *p);
int rm_group_set_n2n_matrix(rm_group *g, int32_t m, const double *row_major);
int rm_group_seed(rm_group *g, int64_t seed);
int rm_group_get_rng_state(rm_group *g, uint64_t *state48);
int rm_group_set_link_capacity(rm_group *g, uint32_t max_links_per_member);
int rm_group_nodes_upload(rm_group *g, int32_t n, const double *x, const double *y, const double *z,
                          const double *txpower, const int32_t *channel, const uint8_t *enabled,
                          const double *rxprob, const double *txprob, const int32_t *int_id);
int rm_group_node_update(rm_group *g, int32_t node, double x, double y, double z, double txpower,
                         int32_t channel, uint8_t enabled, double rxprob, double txprob);
int rm_group_set_time(rm_group *g, int64_t current_time_us);
int rm_group_tick_begin(rm_group *g, int64_t t_begin_us, int64_t t_end_us);
int rm_group_enqueue_tx(rm_group *g, int32_t src, int64_t start_us, int64_t air_us, const double *txpower,
                        const int32_t *channel);
int rm_group_enqueue_tx_records(rm_group *g, const rm_tx_record *recs, int32_t n);
/* as rm_tick_flush, over all members */
int rm_group_tick_flush(rm_group *g, int32_t *pkt, int32_t *dst, uint8_t *verdict, double *rssi, double *sinr,
                        uint32_t cap, uint32_t *count, uint8_t *pkt_interference, uint32_t *pkt_offset);

/* the device-resident tick of a group: dev_src[r] = `slots` source node indices in member r's device memory (the
 * transmitters member r owns, -1 = padding).  Every member packs the Tx records of its transmitters from its resident node
 * state, the members all-gather the packed blocks -- RCCL (ncclAllGather over a communicator from ncclCommInitAll, xGMI
 * between the devices; rm_group_uses_rccl tells) when every member has its own device, copies on the device when several
 * members share one -- and every member sweeps the gathered frames (packet order: member after member, slot after slot)
 * against its receivers.  Nothing crosses PCIe; rm_group_result_copy merges the members' heard links like
 * rm_group_tick_flush, rm_group_context(g, r) + rm_result_device leave them on the devices. */
int rm_group_tick_run_sources_device(rm_group *g, int64_t t_begin_us, int64_t t_end_us, const int32_t *const *dev_src,
                                     int32_t slots, int64_t start_us, int64_t air_us);
int rm_group_result_copy(rm_group *g, int32_t *pkt, int32_t *dst, uint8_t *verdict, double *rssi, double *sinr, uint32_t cap,
                         uint32_t *count, uint8_t *pkt_interference, uint32_t *pkt_offset);
int rm_group_uses_rccl(rm_group *g); /* 1: the members exchange over RCCL, 0: copies on one device, < 0: error */

/* ---- RCCL inside the library: one process per GPU without a framework in between -------------------------------
 * The receiver-sharded tick of SURVEY.md section 8e as ONE call per rank: pack the Tx records of the transmitters this
 * rank owns (from its resident node state), ncclAllGather of the packed blocks over xGMI, sweep of the gathered frames
 * against this rank's receivers (rm_set_partition_spatial / rm_set_partition), all on the context's stream.  RCCL is
 * bound at run time (dlopen: a process that already holds an RCCL shares it; RM_RCCL_LIB names another file);
 * rm_comm_available() tells whether it could be.  Rank 0 makes the id (ncclGetUniqueId) and hands it to the other ranks by
 * whatever means the host has (a file, a socket, MPI, torch.distributed's store); every rank then calls rm_comm_init_rank
 * on its context.  A context without a communicator is a world of one (no collective).
 *   dev_src: n_ticks rows of `slots` source node indices (this rank's transmitters of every tick, -1 = padding).
 *   Packet order of a tick: rank after rank, slot after slot (world * slots packets, padding included).
 * rm_dist_tick_run_sources_device also exchanges the java.util.Random draw counts (regions: the drawing links' nodes)
 * over the same communicator and finishes the draws; it is the form for media with draws and for the SINR medium with
 * frames that stay on the air.  Results: rm_result_* / rm_batch_result_*, as after rm_tick_run_device / rm_batch_run_device. */
#define RM_COMM_ID_BYTES 128
int rm_comm_available(void);
int rm_comm_get_unique_id(uint8_t *id /* [RM_COMM_ID_BYTES] */);
int rm_comm_init_rank(rm_context *ctx, const uint8_t *id, int32_t world, int32_t rank);
int rm_comm_destroy(rm_context *ctx);
int rm_comm_world(const rm_context *ctx);
int rm_comm_rank(const rm_context *ctx);
int rm_dist_batch_run_sources_device(rm_context *ctx, int32_t n_ticks, const int64_t *t_begin_us, const int64_t *t_end_us,
                                     const int32_t *dev_src, int32_t slots, const int64_t *start_us, int64_t air_us);
int rm_dist_tick_run_sources_device(rm_context *ctx, int64_t t_begin_us, int64_t t_end_us, const int32_t *dev_src, int32_t slots,
                                    int64_t start_us, int64_t air_us);

/* ---- reception stage: what the reference does with the verdicts, on the device -------------------------
 * SURVEY.md section 8f-1 / 8f-3.  After rm_events_enable every evaluated tick (rm_transmit, rm_tick_flush*,
 * rm_tick_run*; the ticks of a batch through rm_events_process_batch, below) also hands its packets and heard links to the
 * event stage, exactly as the
 * reference's media call Simulator.generateTransmissionEvents / generateReceptionEvents (Simulator.java:321-350)
 * per packet and heard link: event times max(start, rm_set_time value) and + air time.  The constant-loss
 * medium queues nothing and delivers synchronously (UDGMConstantLossRadioMedium.java:30): its links come
 * out of the next rm_events_process call first, in call order.
 *
 * rm_events_process(t) is Simulator.emulatorTimeStepDone (:155-165): currentTime = t; processAllEvents(t)
 * pops every event with time < t (strict, :213-228) in the order of the reference's ladder queue
 * (com/botbox/scheduler/EventQueue.java; equal timestamps included, see csrc/rm_evorder.hpp) and executes
 * it (events/ReceptionEvent.java:35-46, events/TransmissionEvent.java:18-26, Transciever.java:80-113).  The
 * deliveries -- the Simulator.deliverRadioPacket(packet, destination, rssi) calls of that drain, in call
 * order -- are returned in pinned, host-mapped memory (valid until the next rm_events_process).  Packets are
 * numbered in the order they were handed in since rm_events_enable (rm_events_next_packet tells the number
 * the next one gets; every record of a tick counts, padding records too).
 *
 * rm_node_info gives the per-node fields of a time-step message (net/JSONClientConnection.java:331-341):
 * Transciever.getRSSI (:52-61), getReceivingState (:67-78: 0 listening, 1 transmitting, 2 receiving,
 * 3 disabled) and the wireless channel, from the device-resident radio state; nodes == NULL: nodes 0..n-1.
 * On a receiver partition (rm_set_partition) a context keeps the events of its own nodes only.
 *
 * What the two capacities of rm_events_enable bound (each is rounded up to a power of two, 64 at least; 0: 2^16 packets,
 * 2^21 links).  The pending packets and their heard links live in two rings, and a ring gives room back from its head only:
 *   - a hand-over of a tick of n records (padding records included) with L heard links is refused as a whole if
 *     occupied packets + n > max_pending_packets or occupied links + L > max_pending_links, occupied as the last drain left
 *     it plus what was handed over since; a tick that fills a ring exactly is taken.  A refused tick keeps its packet numbers
 *     (rm_events_next_packet moves on) but leaves no events; the next drain -- and only that one -- returns RM_ERR_CAPACITY,
 *     with its view filled as ever from the packets that are in the rings, which take the next ticks again;
 *   - a packet is finished by the drain that fires its last event (t1 = max(start, current time) + air time < time_us; a
 *     packet of the constant-loss medium by the first drain after its hand-over; a padding record is no packet and is finished
 *     as it is stored);
 *   - a drain first moves the head up to the oldest packet, this tick's included, that was not finished BEFORE this drain (to
 *     the tail if there is none), then fires.  So what a drain finishes is released by the NEXT drain, and only up to the
 *     oldest packet still on the air: one long frame at the head holds every packet handed in after it, finished or not,
 *     and their links.
 * pending_packets is the occupied part of the packet ring after that move, oldest_packet the number of the packet at its
 * head.  To size the rings: the records (links) of every tick handed in while the longest frame is on the air, plus those of
 * the tick before and of one more drain. */
typedef struct rm_delivery_view {
    uint32_t count;            /* deliveries of this drain */
    uint32_t pending_packets;  /* packets in the ring when this drain began to fire: from the oldest one that had events queued
                                * then to the newest, finished ones in between included (the rule above) */
    int64_t oldest_packet;     /* number of the oldest of them (== rm_events_next_packet: none): every packet
                                * below it has fired its last event and may be forgotten by the host */
    const int64_t *packet;     /* NULL since ABI version 3: the packet numbers come once per run (below) */
    const int32_t *dst;        /* [count] destination node index */
    const double *rssi;        /* [count] */
    /* The list in runs: all deliveries of one packet in this drain are adjacent (one fired end group of the queue), so the
     * packet number crosses the link once per run instead of once per delivery (8 of 20 bytes).  Run r covers the
     * deliveries [run_first[r], run_first[r] + run_count[r]); the runs are in list order and cover it completely. */
    uint32_t n_runs;
    const int64_t *run_packet; /* [n_runs] */
    const uint32_t *run_first; /* [n_runs] */
    const uint32_t *run_count; /* [n_runs] */
} rm_delivery_view;
int rm_events_enable(rm_context *ctx, uint32_t max_pending_packets, uint32_t max_pending_links); /* 0, 0: defaults */
int rm_events_disable(rm_context *ctx);
int64_t rm_events_next_packet(rm_context *ctx);
int rm_events_process(rm_context *ctx, int64_t time_us, rm_delivery_view *out);
/* The ticks of the last rm_batch_run_device / rm_batch_run_sources_device call handed to the reception stage, slot b as tick b:
 * identical, bit for bit, to a lone tick's hand-over of slot b (its transmissions at the current time, as rm_set_time or the
 * drain before left it) followed by rm_events_process(time_us[b], &out[b]), for b = 0 .. n_ticks-1.  Afterwards the current
 * time is time_us[n_ticks-1], rm_events_next_packet has moved on by every record of the batch (padding included) and
 * rm_node_info / rm_node_info_changed report the state after the last drain.  All drains are issued at once (no host round
 * trip between ticks); the views point into one host-mapped block, valid until the next rm_events_process* call.
 * RM_ERR_STATE, with nothing changed: events were not on when the batch ran, no batch, the batch was handed over already,
 * or anything that rewrites the slots, the node table or the medium came in between (a lone tick, rm_transmit, another
 * batch, rm_nodes_upload / rm_node_update / rm_nodes_move / rm_set_partition*, rm_set_model / rm_set_n2n_matrix,
 * rm_events_process, rm_events_enable); draws pending; the gathered and rm_dist_* batches and spatially partitioned
 * contexts, which drain one tick at a time.  RM_ERR_INVALID: n_ticks is not the batch's tick count.  RM_ERR_CAPACITY as
 * rm_events_process reports it (a slot that overflowed the link capacity, the pending rings), for the first drain that
 * lost something; every view is filled all the same. */
int rm_events_process_batch(rm_context *ctx, int32_t n_ticks, const int64_t *time_us, rm_delivery_view *out);
int rm_node_info(rm_context *ctx, const int32_t *nodes, int32_t n, double *rssi, int32_t *receiving, int32_t *channel);
/* The same, incrementally (ABI version 4): only the nodes whose (rssi, receiving state, channel) differ from what THIS call
 * reported for them last -- the first call after rm_events_enable or a new node table reports every node.  A time-step
 * message repeats every node's fields each step (net/JSONClientConnection.java:326-353); a host that keeps the text it sent
 * last re-serialises only these.  nodes / rssi / receiving / channel take up to cap entries (cap >= the node count), in no
 * particular order; count gets how many there are. */
int rm_node_info_changed(rm_context *ctx, int32_t *nodes, double *rssi, int32_t *receiving, int32_t *channel, int32_t cap, int32_t *count);

/* ---- host-side helpers exported for tests ------------------------------------------------- */
/* java.util.Random LCG: state after `steps` next() calls */
uint64_t rm_lcg_jump(uint64_t state48, uint64_t steps);
double rm_lcg_next_double(uint64_t *state48);
/* the exact-arithmetic layer of the extension spec as the HOST compiler builds it from the kernels' header
 * (csrc/rm_math.hpp; no device needed): fn 0 det_log2, 1 det_exp2, 2 det_log10, 3 det_pow10, 4 det_normal,
 * 5 Q80 truncation and back; the per-link shadowing hash and its uniform deviate */
double rm_det_math(int32_t fn, double x);
uint64_t rm_link_hash(uint64_t seed, uint32_t a, uint32_t b, double *u);
/* the pop order of the reference's event queue as a sort key (csrc/rm_evorder.hpp; no device needed):
 * rm_evq_add returns the ladder of an event added now with time t, rm_evq_drain is processAllEvents(t) */
typedef struct rm_evq_order {
    int64_t top_start, top_max;
    int32_t ladders, top_nonempty;
} rm_evq_order;
void rm_evq_init(rm_evq_order *o);
int32_t rm_evq_add(rm_evq_order *o, int64_t time_us);
void rm_evq_drain(rm_evq_order *o, int64_t time_us);

#ifdef __cplusplus
}
#endif
#endif /* RADIOMEDIUM_HIP_H */
