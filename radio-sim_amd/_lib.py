"""ctypes binding of libradiomedium_hip.so (include/radiomedium_hip.h).

The library is the product; nothing here computes anything.  Loading fails loudly if the
shared object is missing and cannot be built, and `rm_create` fails loudly without a gfx950
device -- there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.environ.get("RM_LIBRARY") or os.path.join(_CSRC, "libradiomedium_hip.so")  # RM_LIBRARY: a diagnostic build (make stamps)

MODEL_NULL, MODEL_UDGM, MODEL_UDGM_CONST, MODEL_N2N, MODEL_LOGDIST = range(5)
UNHEARD, INTERFERED, DELIVERED = 0, 1, 2
LD_SINR = 1
CHANNEL_OWN = -1
ED_TRANSMITTING, ED_BUSY = 1, 2
CSMA_NONE, CSMA_SENT, CSMA_FAILED, CSMA_PENDING = 0, 1, 2, 3
MAX_BATCH = 512
RM_OK, RM_ERR_INVALID, RM_ERR_NO_DEVICE, RM_ERR_HIP, RM_ERR_CAPACITY, RM_ERR_STATE = 0, -1, -2, -3, -4, -5


class RadioMediumError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("rm error %d: %s" % (code, message))
        self.code = code


class CsmaParams(C.Structure):
    _fields_ = [("max_backoffs", C.c_int32), ("min_be", C.c_int32), ("max_be", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class CsmaResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("attempts", C.c_void_p), ("tick", C.c_void_p), ("pkt", C.c_void_p), ("flags", C.c_void_p),
                ("energy_dbm", C.c_void_p)]


class CsmaCarry(C.Structure):
    """rm_csma_carry: a pending packet on its way into the next CSMA-CA gated batch (24 bytes)"""
    _fields_ = [("origin_cca_time_us", C.c_int64), ("origin_slot", C.c_int32), ("node", C.c_int32), ("tick", C.c_int32),
                ("attempt", C.c_int32)]


class ErrorModel(C.Structure):
    """rm_error_model: the frame error model of the SINR medium (24 bytes)"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("us_per_bit", C.c_double), ("seed", C.c_uint64)]


EM_NONE, EM_OQPSK_250K = 0, 1


class NodeStats(C.Structure):
    """rm_node_stats: one node's traffic counters (64 bytes)"""
    _fields_ = [("tx_frames", C.c_uint64), ("tx_failed", C.c_uint64), ("tx_air_us", C.c_uint64), ("tx_links_heard", C.c_uint64),
                ("tx_links_delivered", C.c_uint64), ("rx_heard", C.c_uint64), ("rx_delivered", C.c_uint64), ("rx_air_us", C.c_uint64)]


class StatsTotals(C.Structure):
    """rm_stats_totals"""
    _fields_ = [("ticks_counted", C.c_uint64), ("ticks_skipped", C.c_uint64)]


class UnicastOut(C.Structure):
    """rm_unicast_out: the output arrays of the unicast outcome query; any may be NULL"""
    _fields_ = [("status", C.c_void_p), ("link", C.c_void_p), ("rssi", C.c_void_p), ("sinr", C.c_void_p), ("reply_src", C.c_void_p)]


UC_NONE, UC_NOT_SENT, UC_UNHEARD, UC_INTERFERED, UC_DELIVERED, UC_LOST = 0, 1, 2, 3, 4, 5
UNICAST_FIELDS = (("status", np.uint8), ("link", np.int32), ("rssi", np.float64), ("sinr", np.float64), ("reply_src", np.int32))
# the neighbour query: directions, the largest K
NB_HEARD_BY, NB_HEARS, NB_MAX_K = 0, 1, 16


class HopsOut(C.Structure):
    """rm_hops_out: the output arrays of the hop query, [n_nodes] each; all but hop may be NULL"""
    _fields_ = [("hop", C.c_void_p), ("parent", C.c_void_p), ("rssi", C.c_void_p), ("children", C.c_void_p)]


class HopsTotals(C.Structure):
    """rm_hops_totals"""
    _fields_ = [("reached", C.c_int32), ("max_hop", C.c_int32), ("roots", C.c_int32), ("reserved", C.c_int32)]


HOPS_FIELDS = (("hop", np.int32), ("parent", np.int32), ("rssi", np.float64), ("children", np.int32))


class RoutesParams(C.Structure):
    """rm_routes_params: the parameters of the route query (40 bytes)"""
    _fields_ = [("direction", C.c_int32), ("kind", C.c_int32), ("us_per_bit", C.c_double), ("air_us", C.c_int64),
                ("min_rssi_dbm", C.c_double), ("max_link_cost", C.c_uint32), ("reserved", C.c_uint32)]


class RoutesOut(C.Structure):
    """rm_routes_out: the output arrays of the route query, [n_nodes] each; all but cost may be NULL"""
    _fields_ = [("cost", C.c_void_p), ("parent", C.c_void_p), ("rssi", C.c_void_p), ("link_cost", C.c_void_p), ("children", C.c_void_p)]


class RoutesTotals(C.Structure):
    """rm_routes_totals"""
    _fields_ = [("reached", C.c_int32), ("roots", C.c_int32), ("max_cost", C.c_uint64)]


ROUTES_FIELDS = (("cost", np.uint64), ("parent", np.int32), ("rssi", np.float64), ("link_cost", np.uint32), ("children", np.int32))
ROUTE_UNREACHED = 0xFFFFFFFFFFFFFFFF

ETX_INBOUND, ETX_BOTH = 0, 1


class EtxTables(C.Structure):
    """rm_etx_tables: a watch table of the measured-route query, peer and stats [n_nodes][K]"""
    _fields_ = [("peer", C.c_void_p), ("stats", C.c_void_p), ("K", C.c_int32), ("reserved", C.c_int32)]


class EtxParams(C.Structure):
    """rm_etx_params (24 bytes)"""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32), ("min_heard", C.c_uint32), ("max_link_cost", C.c_uint32),
                ("hysteresis", C.c_uint32), ("reserved2", C.c_uint32)]


class EtxOut(C.Structure):
    """rm_etx_out: the output arrays of the measured-route query, [n_nodes] each; all but cost may be NULL"""
    _fields_ = [("cost", C.c_void_p), ("parent", C.c_void_p), ("slot", C.c_void_p), ("link_cost", C.c_void_p), ("children", C.c_void_p)]


class EtxTotals(C.Structure):
    """rm_etx_totals"""
    _fields_ = [("reached", C.c_int32), ("roots", C.c_int32), ("kept", C.c_int32), ("switched", C.c_int32), ("lost", C.c_int32),
                ("reserved", C.c_int32), ("max_cost", C.c_uint64)]


assert C.sizeof(EtxParams) == 24 and C.sizeof(EtxTotals) == 32
ETX_FIELDS = (("cost", np.uint64), ("parent", np.int32), ("slot", np.int32), ("link_cost", np.uint32), ("children", np.int32))


class FwdParams(C.Structure):
    """rm_fwd_params: the forwarding queues' parameters (40 bytes)"""
    _fields_ = [("queue_slots", C.c_int32), ("max_retries", C.c_int32), ("min_be", C.c_int32), ("max_be", C.c_int32),
                ("max_hops", C.c_int32), ("reserved", C.c_int32), ("backoff_unit_us", C.c_int64), ("seed", C.c_uint64)]


FWD_NO_ROUTE, FWD_SINK = -1, -2
FWD_NODE_DTYPE = np.dtype([(f, "<u8") for f in ("generated", "arrived", "lost", "latency_us_sum", "latency_us_max", "hops_sum", "attempts",
                                                "acked", "failed", "deferred", "rejected", "dropped")] +
                          [("ready_us", "<i8"), ("next", "<i4"), ("queue_len", "<i4"), ("queue_max", "<i4"), ("tries", "<i4"),
                           ("slot_mask", "<u4"), ("reserved", "<u4")])
FWD_PACKET_DTYPE = np.dtype([("origin", "<i4"), ("hops", "<i4"), ("birth_us", "<i8"), ("enq_us", "<i8")])
FWD_TOTALS_DTYPE = np.dtype([(f, "<u8") for f in ("generated", "arrived", "dropped_retries", "dropped_no_route", "dropped_full", "dropped_ttl",
                                                  "in_flight", "stray", "skipped_slots", "latency_us_sum", "hops_sum")])
assert C.sizeof(FwdParams) == 40 and FWD_NODE_DTYPE.itemsize == 128 and FWD_PACKET_DTYPE.itemsize == 24 and FWD_TOTALS_DTYPE.itemsize == 88

class FloodParams(C.Structure):
    """rm_flood_params: the dissemination floods' parameters (32 bytes)"""
    _fields_ = [("imin_us", C.c_int64), ("doublings", C.c_int32), ("max_intervals", C.c_int32), ("redundancy", C.c_int32),
                ("max_hops", C.c_int32), ("seed", C.c_uint64)]


FLOOD_NODE_DTYPE = np.dtype([("first_us", "<i8"), ("start_us", "<i8"), ("fire_us", "<i8"), ("rssi_bits", "<u8"), ("parent", "<i4"), ("hop", "<i4"),
                             ("interval", "<i4"), ("c", "<i4"), ("sent", "<u4"), ("suppressed", "<u4"), ("heard", "<u4"), ("deferred", "<u4")])
FLOOD_TOTALS_DTYPE = np.dtype([(f, "<u8") for f in ("covered", "seeds", "sent", "suppressed", "heard", "deferred", "stray", "skipped_slots",
                                                    "max_hop", "last_first_us")])
assert C.sizeof(FloodParams) == 32 and FLOOD_NODE_DTYPE.itemsize == 64 and FLOOD_TOTALS_DTYPE.itemsize == 80


class NbTableParams(C.Structure):
    """rm_nbtable_params: the neighbour tables' parameters (32 bytes)"""
    _fields_ = [("admit_rssi_dbm", C.c_double), ("timeout_us", C.c_int64), ("min_heard", C.c_uint32), ("evict_cost", C.c_uint32),
                ("require_delivered", C.c_int32), ("reserved", C.c_int32)]


NBTABLE_NODE_DTYPE = np.dtype([(f, "<u4") for f in ("admitted", "evicted_stale", "evicted_poor", "refused", "expired")] + [("reserved", "<u4", (3,))])
NBTABLE_TOTALS_DTYPE = np.dtype([(f, "<u8") for f in ("updates", "skipped_slots", "admitted", "evicted_stale", "evicted_poor", "refused", "expired",
                                                      "reserved")])
assert C.sizeof(NbTableParams) == 32 and NBTABLE_NODE_DTYPE.itemsize == 32 and NBTABLE_TOTALS_DTYPE.itemsize == 64


class LinkEstParams(C.Structure):
    """rm_linkest_params: the link estimator's parameters (24 bytes)"""
    _fields_ = [("beacon_window", C.c_uint32), ("data_window", C.c_uint32), ("beacon_alpha_q8", C.c_uint32), ("data_alpha_q8", C.c_uint32),
                ("max_etx", C.c_uint32), ("reserved", C.c_uint32)]


class LinkEstInputs(C.Structure):
    """rm_linkest_inputs: the tables a fold reads -- peer and stats [n_nodes][K], fwd [n_nodes] or NULL"""
    _fields_ = [("peer", C.c_void_p), ("stats", C.c_void_p), ("fwd", C.c_void_p), ("K", C.c_int32), ("reserved", C.c_int32)]


LINKEST_ENTRY_DTYPE = np.dtype([("base_heard", "<u8"), ("base_delivered", "<u8"), ("etx", "<u4"), ("windows", "<u4"), ("data_windows", "<u4"),
                                ("peer", "<i4")])
LINKEST_NODE_DTYPE = np.dtype([("base_tx", "<u8"), ("base_ack", "<u8"), ("base_next", "<i4"), ("data_samples", "<u4"), ("data_unmatched", "<u4"),
                               ("restarted", "<u4")])
LINKEST_TOTALS_DTYPE = np.dtype([(f, "<u8") for f in ("folds", "beacon_samples", "data_samples", "data_unmatched", "restarted", "cleared", "estimates",
                                                      "reserved")])
assert C.sizeof(LinkEstParams) == 24 and LINKEST_ENTRY_DTYPE.itemsize == 32 and LINKEST_NODE_DTYPE.itemsize == 32
assert LINKEST_TOTALS_DTYPE.itemsize == 64

NODE_STATS_DTYPE = np.dtype([(name, "<u8") for name, _ in NodeStats._fields_])
assert NODE_STATS_DTYPE.itemsize == C.sizeof(NodeStats) == 64


class ListenSchedule(C.Structure):
    """rm_listen_schedule: one receiver's listening schedule (24 bytes)"""
    _fields_ = [("period_us", C.c_int64), ("on_us", C.c_int64), ("phase_us", C.c_int64)]


LISTEN_SCHEDULE_DTYPE = np.dtype([(name, "<i8") for name, _ in ListenSchedule._fields_])
assert LISTEN_SCHEDULE_DTYPE.itemsize == C.sizeof(ListenSchedule) == 24


class LinkStats(C.Structure):
    """rm_link_stats: one watched (node, peer) link's counters (48 bytes)"""
    _fields_ = [("heard", C.c_uint64), ("delivered", C.c_uint64), ("rssi_q8_sum", C.c_int64), ("sinr_q8_sum", C.c_int64),
                ("first_start_us", C.c_int64), ("last_start_us", C.c_int64)]


LINK_STATS_DTYPE = np.dtype([(name, "<u8" if t is C.c_uint64 else "<i8") for name, t in LinkStats._fields_])
assert LINK_STATS_DTYPE.itemsize == C.sizeof(LinkStats) == 48


class TrafficSchedule(C.Structure):
    """rm_traffic_schedule: one node's periodic traffic (32 bytes)"""
    _fields_ = [("period_us", C.c_int64), ("phase_us", C.c_int64), ("jitter_us", C.c_int64), ("reserved", C.c_int64)]


TRAFFIC_SCHEDULE_DTYPE = np.dtype([(name, "<i8") for name, _ in TrafficSchedule._fields_])
assert TRAFFIC_SCHEDULE_DTYPE.itemsize == C.sizeof(TrafficSchedule) == 32


class TrafficTotals(C.Structure):
    """rm_traffic_totals: what one generate counted"""
    _fields_ = [("packets", C.c_uint64), ("coalesced", C.c_uint64), ("truncated", C.c_uint64)]


class ModelParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32),
                ("udgm_success_ratio_tx", C.c_double), ("udgm_success_ratio_rx", C.c_double),
                ("udgm_transmission_range", C.c_double), ("udgm_interference_range", C.c_double),
                ("const_range", C.c_double),
                ("ld_pl0_db", C.c_double), ("ld_exponent", C.c_double), ("ld_d0", C.c_double),
                ("ld_sigma_db", C.c_double), ("ld_clip", C.c_double), ("ld_seed", C.c_uint64),
                ("ld_sensitivity_dbm", C.c_double), ("ld_noise_dbm", C.c_double),
                ("ld_capture_db", C.c_double), ("ld_ifloor_dbm", C.c_double)]


class TxRecord(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double),
                ("txpower", C.c_double), ("txprob", C.c_double),
                ("start_us", C.c_int64), ("air_us", C.c_int64),
                ("src", C.c_int32), ("channel", C.c_int32)]


TX_RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("txpower", "<f8"), ("txprob", "<f8"),
                            ("start_us", "<i8"), ("air_us", "<i8"), ("src", "<i4"), ("channel", "<i4")])
assert TX_RECORD_DTYPE.itemsize == C.sizeof(TxRecord) == 64


class DeviceResult(C.Structure):
    _fields_ = [("count", C.c_void_p), ("pkt_offset", C.c_void_p), ("pkt", C.c_void_p), ("dst", C.c_void_p),
                ("verdict", C.c_void_p), ("rssi", C.c_void_p), ("sinr", C.c_void_p), ("capacity", C.c_uint32)]


class DenseResult(C.Structure):
    """rm_dense_result"""
    _fields_ = [("cell_mask", C.c_void_p), ("cell_count", C.c_void_p), ("count", C.c_void_p), ("pkt_offset", C.c_void_p),
                ("pkt_interference", C.c_void_p), ("n_packets", C.c_int32), ("chunks", C.c_int32), ("rx_first", C.c_int32)]


class KernelTime(C.Structure):
    """rm_kernel_time"""
    _fields_ = [("name", C.c_char * 96), ("stage", C.c_int32), ("launches", C.c_uint32), ("total_ms", C.c_double)]


class HostResult(C.Structure):
    _fields_ = [("count", C.c_uint32), ("n_packets", C.c_uint32), ("pkt_offset", C.c_void_p),
                ("pkt_interference", C.c_void_p), ("pkt", C.c_void_p), ("dst", C.c_void_p), ("verdict", C.c_void_p),
                ("rssi", C.c_void_p), ("sinr", C.c_void_p), ("pkt_rssi", C.c_void_p)]


class DeliveryView(C.Structure):
    _fields_ = [("count", C.c_uint32), ("pending_packets", C.c_uint32), ("oldest_packet", C.c_int64), ("packet", C.c_void_p), ("dst", C.c_void_p),
                ("rssi", C.c_void_p), ("n_runs", C.c_uint32), ("run_packet", C.c_void_p), ("run_first", C.c_void_p), ("run_count", C.c_void_p)]


class EvqOrder(C.Structure):
    _fields_ = [("top_start", C.c_int64), ("top_max", C.c_int64), ("ladders", C.c_int32), ("top_nonempty", C.c_int32)]


def library_path():
    return _SO


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".cpp", ".h", ".hpp")) or f == "Makefile"]
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "radiomedium_hip.h"))
    stale = (not os.path.exists(_SO)) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _CSRC, "-s", "-j4", "libradiomedium_hip.so"])
    return _SO


_lib = None

# name -> (restype, argtypes); every entry point declared in include/radiomedium_hip.h
SIGNATURES = {
    "rm_abi_version": (C.c_int, []),
    "rm_device_count": (C.c_int, []),
    "rm_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "rm_destroy": (None, [C.c_void_p]),
    "rm_last_error": (C.c_char_p, []),
    "rm_get_name": (C.c_char_p, [C.c_void_p]),
    "rm_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rm_model_defaults": (None, [C.POINTER(ModelParams), C.c_int32]),
    "rm_set_model": (C.c_int, [C.c_void_p, C.POINTER(ModelParams)]),
    "rm_get_model": (C.c_int, [C.c_void_p, C.POINTER(ModelParams)]),
    "rm_set_n2n_matrix": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_set_base_rssi": (C.c_int, [C.c_void_p, C.c_double]),
    "rm_get_base_rssi": (C.c_double, [C.c_void_p, C.c_int32]),
    "rm_seed": (C.c_int, [C.c_void_p, C.c_int64]),
    "rm_get_rng_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rm_set_rng_state": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rm_nodes_upload": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 9),
    "rm_node_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_int32, C.c_uint8, C.c_double, C.c_double]),
    "rm_receiver_table_builds": (C.c_int64, [C.c_void_p]),
    "rm_nodes_move": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_node_count": (C.c_int, [C.c_void_p]),
    "rm_set_partition": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rm_set_partition_spatial": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rm_partition_of_nodes": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_region_split": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_partition_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "rm_set_link_capacity": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rm_set_time": (C.c_int, [C.c_void_p, C.c_int64]),
    "rm_air_time_us": (C.c_int64, [C.c_int64]),
    "rm_event_times": (None, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rm_transmit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_double),
                              C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    "rm_tick_begin": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    "rm_enqueue_tx": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_double),
                                C.POINTER(C.c_int32)]),
    "rm_enqueue_tx_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rm_tick_flush": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "rm_batch_result_view": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_tick_flush_view": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rm_tick_run": (C.c_int, [C.c_void_p]),
    "rm_draws_pending": (C.c_int, [C.c_void_p]),
    "rm_draw_counts_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "rm_draw_counts_to": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rm_tick_finish_draws": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int]),
    "rm_draw_nodes_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rm_tick_finish_draws_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int]),
    "rm_pack_tx_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    "rm_pack_tx_device_on": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    "rm_pack_tx_batch_device_on": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                             C.c_void_p]),
    "rm_tick_run_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
    "rm_tick_run_records_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_tick_run_sources_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                             C.c_int64]),
    "rm_result_device": (C.c_int, [C.c_void_p, C.POINTER(DeviceResult)]),
    "rm_result_dense": (C.c_int, [C.c_void_p, C.POINTER(DenseResult)]),
    "rm_result_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rm_result_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                 C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "rm_sync": (C.c_int, [C.c_void_p]),
    "rm_batch_run_sources_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "rm_batch_run_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_batch_run_gathered_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "rm_batch_run_gathered_sources_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "rm_batch_run_gathered_blocks_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]),
    "rm_table_digest": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rm_batch_tile_reuse": (C.c_int, [C.c_void_p]),
    "rm_comm_available": (C.c_int, []),
    "rm_comm_get_unique_id": (C.c_int, [C.c_void_p]),
    "rm_comm_init_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "rm_comm_destroy": (C.c_int, [C.c_void_p]),
    "rm_comm_world": (C.c_int, [C.c_void_p]),
    "rm_comm_rank": (C.c_int, [C.c_void_p]),
    "rm_dist_batch_run_sources_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                   C.c_int64]),
    "rm_dist_tick_run_sources_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    "rm_group_tick_run_sources_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    "rm_group_result_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "rm_group_uses_rccl": (C.c_int, [C.c_void_p]),
    "rm_batch_result_device": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(DeviceResult)]),
    "rm_batch_result_count": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rm_batch_result_copy": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "rm_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "rm_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
    "rm_profile_kernels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "rm_last_link_evaluations": (C.c_int64, [C.c_void_p]),
    "rm_slot_stats": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rm_air_ring_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rm_air_list_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rm_air_scan_ticks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rm_air_batch_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rm_air_batch_pairs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rm_group_create": (C.c_int, [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rm_group_destroy": (None, [C.c_void_p]),
    "rm_group_size": (C.c_int, [C.c_void_p]),
    "rm_group_set_partitioning": (C.c_int, [C.c_void_p, C.c_int32]),
    "rm_group_context": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "rm_group_set_model": (C.c_int, [C.c_void_p, C.POINTER(ModelParams)]),
    "rm_group_set_n2n_matrix": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_group_seed": (C.c_int, [C.c_void_p, C.c_int64]),
    "rm_group_get_rng_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rm_group_set_link_capacity": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rm_group_nodes_upload": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 9),
    "rm_group_node_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.c_int32, C.c_uint8, C.c_double, C.c_double]),
    "rm_group_set_time": (C.c_int, [C.c_void_p, C.c_int64]),
    "rm_group_tick_begin": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    "rm_group_enqueue_tx": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_double),
                                      C.POINTER(C.c_int32)]),
    "rm_group_enqueue_tx_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "rm_group_tick_flush": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]),
    "rm_events_enable": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rm_events_disable": (C.c_int, [C.c_void_p]),
    "rm_events_next_packet": (C.c_int64, [C.c_void_p]),
    "rm_events_process": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "rm_events_process_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_node_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_node_info_changed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "rm_channel_energy_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "rm_channel_energy": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "rm_tick_run_sources_cca_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                                 C.c_double, C.c_void_p, C.c_void_p]),
    "rm_tick_run_sources_cca": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_double, C.c_void_p, C.c_void_p]),
    "rm_batch_run_sources_cca_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "rm_batch_run_sources_cca": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "rm_csma_defaults": (None, [C.c_void_p]),
    "rm_csma_schedule": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.POINTER(C.c_int64)]),
    "rm_batch_run_sources_csma_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_batch_run_sources_csma": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_csma_schedule_carry": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_batch_run_sources_csma_carry_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_int32, C.c_void_p]),
    "rm_batch_run_sources_csma_carry": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                  C.c_void_p]),
    "rm_csma_carry_collect": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_csma_carry_collect_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_error_model_defaults": (None, [C.c_void_p, C.c_int32]),
    "rm_set_error_model": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rm_get_error_model": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rm_error_model_psr": (C.c_double, [C.c_void_p, C.c_double, C.c_int64]),
    "rm_error_model_draw": (C.c_double, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32]),
    "rm_stats_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "rm_stats_enabled": (C.c_int, [C.c_void_p]),
    "rm_stats_reset": (C.c_int, [C.c_void_p]),
    "rm_stats_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(StatsTotals)]),
    "rm_stats_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_unicast_query_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_unicast_query": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_unicast_query_at_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_unicast_query_at": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_unicast_from_result": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_listen_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_listen_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_listen_clear": (C.c_int, [C.c_void_p]),
    "rm_listen_enabled": (C.c_int, [C.c_void_p]),
    "rm_listen_missed_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_listen_missed_reset": (C.c_int, [C.c_void_p]),
    "rm_listen_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_listen_at": (C.c_int, [C.c_void_p, C.c_int64]),
    "rm_linkstats_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "rm_linkstats_enabled": (C.c_int, [C.c_void_p]),
    "rm_linkstats_watch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_linkstats_peers_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_linkstats_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(StatsTotals)]),
    "rm_linkstats_reset": (C.c_int, [C.c_void_p]),
    "rm_linkstats_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_linkstats_q8": (C.c_int64, [C.c_double]),
    "rm_linkstats_validate": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_traffic_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_traffic_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_traffic_clear": (C.c_int, [C.c_void_p]),
    "rm_traffic_enabled": (C.c_int, [C.c_void_p]),
    "rm_traffic_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rm_traffic_generate_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "rm_traffic_generate": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_traffic_due": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "rm_traffic_validate": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_neighbors_query_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_neighbors_query": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_neighbors_from_result": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_linkstats_watch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_linkstats_stage_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rm_hops_query_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.POINTER(HopsOut), C.POINTER(HopsTotals)]),
    "rm_hops_query": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.POINTER(HopsOut), C.POINTER(HopsTotals)]),
    "rm_hops_next_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "rm_hops_from_links": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                     C.POINTER(HopsOut), C.POINTER(HopsTotals)]),
    "rm_routes_query_device": (C.c_int, [C.c_void_p, C.POINTER(RoutesParams), C.c_void_p, C.c_int32, C.POINTER(RoutesOut), C.POINTER(RoutesTotals)]),
    "rm_routes_query": (C.c_int, [C.c_void_p, C.POINTER(RoutesParams), C.c_void_p, C.c_int32, C.POINTER(RoutesOut), C.POINTER(RoutesTotals)]),
    "rm_routes_last_work": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "rm_routes_link_cost": (C.c_int, [C.POINTER(RoutesParams), C.c_double, C.c_double, C.POINTER(C.c_uint32)]),
    "rm_routes_from_links": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RoutesParams), C.c_double, C.c_void_p,
                                       C.c_int32, C.POINTER(RoutesOut), C.POINTER(RoutesTotals)]),
    "rm_etx_defaults": (None, [C.POINTER(EtxParams)]),
    "rm_etx_validate": (C.c_int, [C.POINTER(EtxParams)]),
    "rm_etx_query_device": (C.c_int, [C.c_void_p, C.POINTER(EtxParams), C.POINTER(EtxTables), C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(EtxOut),
                                      C.POINTER(EtxTotals)]),
    "rm_etx_query": (C.c_int, [C.c_void_p, C.POINTER(EtxParams), C.POINTER(EtxTables), C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(EtxOut),
                               C.POINTER(EtxTotals)]),
    "rm_etx_last_work": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "rm_etx_link_cost": (C.c_int, [C.POINTER(EtxParams), C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]),
    "rm_etx_combine": (C.c_uint64, [C.c_uint32, C.c_uint32]),
    "rm_etx_from_tables": (C.c_int, [C.c_int32, C.POINTER(EtxTables), C.POINTER(EtxParams), C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(EtxOut),
                                     C.POINTER(EtxTotals)]),
    "rm_fwd_defaults": (None, [C.POINTER(FwdParams)]),
    "rm_fwd_validate": (C.c_int, [C.POINTER(FwdParams)]),
    "rm_fwd_backoff": (C.c_int, [C.POINTER(FwdParams), C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "rm_fwd_enable": (C.c_int, [C.c_void_p, C.POINTER(FwdParams)]),
    "rm_fwd_disable": (C.c_int, [C.c_void_p]),
    "rm_fwd_enabled": (C.c_int, [C.c_void_p]),
    "rm_fwd_get_params": (C.c_int, [C.c_void_p, C.POINTER(FwdParams)]),
    "rm_fwd_reset": (C.c_int, [C.c_void_p]),
    "rm_fwd_set_next_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_fwd_set_next": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_fwd_inject_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_fwd_inject": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_fwd_sources_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_fwd_sources": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "rm_fwd_advance_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "rm_fwd_advance": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "rm_fwd_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_fwd_queue_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_fwd_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_flood_defaults": (None, [C.POINTER(FloodParams)]),
    "rm_flood_validate": (C.c_int, [C.POINTER(FloodParams)]),
    "rm_flood_fire": (C.c_int, [C.POINTER(FloodParams), C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rm_flood_enable": (C.c_int, [C.c_void_p, C.POINTER(FloodParams)]),
    "rm_flood_disable": (C.c_int, [C.c_void_p]),
    "rm_flood_enabled": (C.c_int, [C.c_void_p]),
    "rm_flood_get_params": (C.c_int, [C.c_void_p, C.POINTER(FloodParams)]),
    "rm_flood_reset": (C.c_int, [C.c_void_p]),
    "rm_flood_seed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_flood_seed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "rm_flood_sources_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_flood_sources": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "rm_flood_advance_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "rm_flood_advance": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "rm_flood_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_flood_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_flood_tree_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_nbtable_defaults": (None, [C.POINTER(NbTableParams)]),
    "rm_nbtable_validate": (C.c_int, [C.POINTER(NbTableParams)]),
    "rm_nbtable_enable": (C.c_int, [C.c_void_p, C.POINTER(NbTableParams)]),
    "rm_nbtable_disable": (C.c_int, [C.c_void_p]),
    "rm_nbtable_enabled": (C.c_int, [C.c_void_p]),
    "rm_nbtable_get_params": (C.c_int, [C.c_void_p, C.POINTER(NbTableParams)]),
    "rm_nbtable_reset": (C.c_int, [C.c_void_p]),
    "rm_nbtable_update_device": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "rm_nbtable_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p]),
    "rm_nbtable_expire_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "rm_nbtable_expire": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "rm_nbtable_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "rm_nbtable_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_nbtable_from_result": (C.c_int, [C.POINTER(HostResult), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.POINTER(NbTableParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_nbtable_expire_tables": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NbTableParams), C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rm_linkest_defaults": (None, [C.POINTER(LinkEstParams)]),
    "rm_linkest_validate": (C.c_int, [C.POINTER(LinkEstParams)]),
    "rm_linkest_enable": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(LinkEstParams)]),
    "rm_linkest_disable": (C.c_int, [C.c_void_p]),
    "rm_linkest_enabled": (C.c_int, [C.c_void_p]),
    "rm_linkest_get_params": (C.c_int, [C.c_void_p, C.POINTER(LinkEstParams)]),
    "rm_linkest_reset": (C.c_int, [C.c_void_p]),
    "rm_linkest_fold_device": (C.c_int, [C.c_void_p, C.POINTER(LinkEstInputs)]),
    "rm_linkest_fold": (C.c_int, [C.c_void_p, C.POINTER(LinkEstInputs)]),
    "rm_linkest_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rm_linkest_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "rm_linkest_tables": (C.c_int, [C.c_void_p, C.POINTER(EtxTables)]),
    "rm_linkest_fold_tables": (C.c_int, [C.c_int32, C.POINTER(LinkEstInputs), C.POINTER(LinkEstParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "rm_det_math": (C.c_double, [C.c_int32, C.c_double]),
    "rm_link_hash": (C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "rm_evq_init": (None, [C.c_void_p]),
    "rm_evq_add": (C.c_int32, [C.c_void_p, C.c_int64]),
    "rm_evq_drain": (None, [C.c_void_p, C.c_int64]),
    "rm_lcg_jump": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "rm_lcg_next_double": (C.c_double, [C.POINTER(C.c_uint64)]),
}


def lib():
    """Load (building first if needed) the HIP library.  Raises if it cannot be had."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build_library()
        L = C.CDLL(_SO)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)  # AttributeError = the library does not match the header
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != RM_OK:
        raise RadioMediumError(code, lib().rm_last_error().decode("utf-8", "replace"))
    return code
