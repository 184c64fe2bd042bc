"""Object wrapper over one rm_context of libradiomedium_hip.so (no computation here)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ModelParams, DeviceResult, HostResult, TX_RECORD_DTYPE, check


def _ptr(a):
    return None if a is None else a.ctypes.data


_CHAR_BLOCKS = {}


def _wrap(ptr, dtype, count):
    """`count` items of `dtype` at address `ptr`, wrapped in place.  ctypes builds (and keeps) a new array type for
    every distinct length -- tens of microseconds each -- so the wrapper's byte length is rounded up to a power of two
    (numpy only ever looks at the first `count` items)."""
    if count == 0 or not ptr:
        return np.empty(0, dtype=dtype)
    nbytes = count * np.dtype(dtype).itemsize
    size = 1 << max(6, (nbytes - 1).bit_length())
    block = _CHAR_BLOCKS.get(size)
    if block is None:
        block = _CHAR_BLOCKS[size] = C.c_char * size
    return np.frombuffer(block.from_address(ptr), dtype=dtype, count=count)


class TickResult:
    """Heard links of one evaluated tick, packet-major / receiver ascending."""

    def __init__(self, count, pkt, dst, verdict, rssi, sinr, pkt_interference, pkt_offset):
        self.count = count
        self.pkt, self.dst, self.verdict, self.rssi, self.sinr = pkt, dst, verdict, rssi, sinr
        self.pkt_interference, self.pkt_offset = pkt_interference, pkt_offset


class HostTickView:
    """The same fields as TickResult over the engine's pinned host block, each wrapped in place the first time it is read
    (a host loop that only looks at a count or two columns does not pay for seven array wrappers per tick)."""
    _FIELDS = {"pkt": ("pkt", np.int32, 0), "dst": ("dst", np.int32, 0), "verdict": ("verdict", np.uint8, 0),
               "rssi": ("rssi", np.float64, 0), "sinr": ("sinr", np.float64, 0),
               "pkt_interference": ("pkt_interference", np.uint8, 1), "pkt_offset": ("pkt_offset", np.uint32, 2)}

    def __init__(self, r):
        self.count = r.count
        self._n_packets = r.n_packets
        self._ptr = {k: getattr(r, v[0]) for k, v in self._FIELDS.items()}
        self._pkt_rssi = r.pkt_rssi   # (ABI version 5) the reference's media: one rssi per packet, no per-link column

    def __getattr__(self, name):
        spec = HostTickView._FIELDS.get(name)
        if spec is None:
            raise AttributeError(name)
        n = (self.count, self._n_packets, self._n_packets + 1)[spec[2]]
        p = self._ptr[name]
        if name == "pkt" and not p:   # (the block carries no packet column since ABI version 3: it follows from the offsets)
            off = self.pkt_offset.astype(np.int64)
            a = np.repeat(np.arange(self._n_packets, dtype=np.int32), np.diff(off))[:n]
        elif name == "rssi" and not p:   # (one value per packet crossed the link: a link's rssi is its packet's transmit power)
            per_pkt = _wrap(self._pkt_rssi, np.float64, self._n_packets) if self._n_packets else np.zeros(0)
            a = np.repeat(per_pkt, np.diff(self.pkt_offset.astype(np.int64)))[:n]
        else:
            a = np.zeros(n) if (name == "sinr" and not p) else _wrap(p, spec[1], n)
        setattr(self, name, a)
        return a


class Engine:
    """One GPU context == one Simulator's radio medium (RadioMedium.java:35-45)."""

    def __init__(self, device=0):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.rm_create(device, C.byref(h)))
        self._h = h
        self.n = 0
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            self._L.rm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- RadioMedium.getName / getBaseRSSI
    def get_name(self):
        return self._L.rm_get_name(self._h).decode()

    def get_base_rssi(self, node=0):
        return self._L.rm_get_base_rssi(self._h, node)

    def set_base_rssi(self, v):
        check(self._L.rm_set_base_rssi(self._h, v))

    # -- model
    @staticmethod
    def default_params(kind):
        p = ModelParams()
        _lib.lib().rm_model_defaults(C.byref(p), kind)
        return p

    def set_model(self, kind, **kw):
        p = self.default_params(kind)
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        check(self._L.rm_set_model(self._h, C.byref(p)))
        return p

    def set_n2n_matrix(self, m):
        m = np.ascontiguousarray(m, dtype=np.float64)
        assert m.ndim == 2 and m.shape[0] == m.shape[1]
        check(self._L.rm_set_n2n_matrix(self._h, m.shape[0], m.ctypes.data))

    # -- frame error model of the SINR medium
    @staticmethod
    def error_model(kind=_lib.EM_OQPSK_250K, us_per_bit=4.0, seed=0, reserved=0):
        """rm_error_model: the library's defaults with the given fields"""
        e = _lib.ErrorModel()
        _lib.lib().rm_error_model_defaults(C.byref(e), kind)
        e.us_per_bit, e.seed, e.reserved = us_per_bit, seed, reserved
        return e

    def set_error_model(self, kind, us_per_bit=4.0, seed=0, reserved=0):
        """rm_set_error_model: EM_NONE switches it off (and so does set_model)"""
        e = self.error_model(kind, us_per_bit, seed, reserved)
        check(self._L.rm_set_error_model(self._h, C.byref(e)))
        return e

    def get_error_model(self):
        e = _lib.ErrorModel()
        check(self._L.rm_get_error_model(self._h, C.byref(e)))
        return e

    @staticmethod
    def error_model_psr(sinr_db, air_us, kind=_lib.EM_OQPSK_250K, us_per_bit=4.0):
        """rm_error_model_psr: the packet success ratio, on the host alone"""
        e = Engine.error_model(kind, us_per_bit)
        return _lib.lib().rm_error_model_psr(C.byref(e), sinr_db, air_us)

    @staticmethod
    def error_model_draw(src, start_us, dst, seed=0):
        """rm_error_model_draw: the link's uniform deviate, on the host alone"""
        e = Engine.error_model(seed=seed)
        return _lib.lib().rm_error_model_draw(C.byref(e), src, start_us, dst)

    # -- what the calls of E11, E13, E14 and E15 that take "a node list, or the whole table" share
    def _node_list(self, nodes):
        """(pointer of the int32 list or None for all nodes in node order, n, the index array to keep alive)"""
        if nodes is None:
            return None, max(int(self._L.rm_node_count(self._h)), 0), None
        idx = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        return idx.ctypes.data, idx.shape[0], idx

    # -- per-node traffic counters accumulated on the device
    def stats_enable(self, on=True):
        """rm_stats_enable: count from the next evaluating call (False: stop counting, the table is kept)"""
        check(self._L.rm_stats_enable(self._h, 1 if on else 0))

    def stats_enabled(self):
        return bool(self._L.rm_stats_enabled(self._h))

    def stats_reset(self):
        check(self._L.rm_stats_reset(self._h))

    def stats_read(self, nodes=None):
        """rm_stats_read: (structured array of NODE_STATS_DTYPE -- the listed nodes in list order, or all in node order --,
        {"ticks_counted": .., "ticks_skipped": ..})"""
        tot = _lib.StatsTotals()
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=_lib.NODE_STATS_DTYPE)
        check(self._L.rm_stats_read(self._h, ptr, n, out.ctypes.data, C.byref(tot)))
        return out, {"ticks_counted": int(tot.ticks_counted), "ticks_skipped": int(tot.ticks_skipped)}

    def stats_device(self):
        """rm_stats_device: (device pointer of the table [n_nodes] of 64-byte records, device pointer of the totals)"""
        tbl, tot = C.c_void_p(), C.c_void_p()
        check(self._L.rm_stats_device(self._h, C.byref(tbl), C.byref(tot)))
        return tbl.value, tot.value

    # -- unicast outcome query: did a frame reach its destination
    UC_NONE, UC_NOT_SENT, UC_UNHEARD, UC_INTERFERED = _lib.UC_NONE, _lib.UC_NOT_SENT, _lib.UC_UNHEARD, _lib.UC_INTERFERED
    UC_DELIVERED, UC_LOST = _lib.UC_DELIVERED, _lib.UC_LOST

    @staticmethod
    def _unicast_host_out(n, fields):
        """host arrays for n entries -> (rm_unicast_out, {name: array}); fields: the outputs asked for (None: all five)"""
        arrs = {name: np.empty(n, dtype=dt) for name, dt in _lib.UNICAST_FIELDS if fields is None or name in fields}
        return _lib.UnicastOut(**{name: a.ctypes.data for name, a in arrs.items()}), arrs

    @staticmethod
    def _unicast_dev_out(dev_out):
        if isinstance(dev_out, _lib.UnicastOut):
            return dev_out
        return _lib.UnicastOut(**{name: (int(p) if p else None) for name, p in dev_out.items()})

    def unicast_query(self, want_lists, fields=None):
        """rm_unicast_query: want_lists[b][p] is the wanted node of packet p of result slot b (-1: not asked) -> dict of flat
        numpy arrays status / link / rssi / sinr / reply_src, in slot order"""
        lists = [np.ascontiguousarray(w, dtype=np.int32).reshape(-1) for w in want_lists]
        n_pkt = np.array([len(w) for w in lists], dtype=np.int32)
        want = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.int32)
        out, arrs = self._unicast_host_out(len(want), fields)
        check(self._L.rm_unicast_query(self._h, len(lists), n_pkt.ctypes.data, want.ctypes.data, C.byref(out)))
        return arrs

    def unicast_query_device(self, n_pkt, dev_want_ptr, dev_out):
        """rm_unicast_query_device: n_pkt[b] entries per slot (host), the wanted nodes and the outputs in device memory
        (dev_out: a dict name -> device pointer, or a _lib.UnicastOut); enqueued on the context's stream, not waited for"""
        n_pkt = np.ascontiguousarray(n_pkt, dtype=np.int32)
        out = self._unicast_dev_out(dev_out)
        check(self._L.rm_unicast_query_device(self._h, len(n_pkt), n_pkt.ctypes.data, dev_want_ptr, C.byref(out)))

    def unicast_query_at(self, slot, pkt, want, fields=None):
        """rm_unicast_query_at: entry e names (slot[e], pkt[e]) -- the tick / pkt columns of a CSMA-CA result -- and want[e]"""
        slot, pkt, want = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (slot, pkt, want))
        assert len(slot) == len(pkt) == len(want)
        out, arrs = self._unicast_host_out(len(want), fields)
        check(self._L.rm_unicast_query_at(self._h, len(want), slot.ctypes.data, pkt.ctypes.data, want.ctypes.data, C.byref(out)))
        return arrs

    def unicast_query_at_device(self, n, dev_slot_ptr, dev_pkt_ptr, dev_want_ptr, dev_out):
        out = self._unicast_dev_out(dev_out)
        check(self._L.rm_unicast_query_at_device(self._h, n, dev_slot_ptr, dev_pkt_ptr, dev_want_ptr, C.byref(out)))

    @staticmethod
    def _host_result(result, keep):
        """a _lib.HostResult as it is, or one over anything with pkt_offset, dst, verdict and rssi or pkt_rssi (sinr optional), e.g.
        what tick_flush_view returns; the arrays it points into are appended to `keep`"""
        if isinstance(result, HostResult):
            return result

        def col(name, dt):
            a = getattr(result, name, None)
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data
        off = np.ascontiguousarray(result.pkt_offset, dtype=np.uint32)
        keep.append(off)
        rssi = col("rssi", np.float64)
        return HostResult(count=int(result.count), n_packets=len(off) - 1, pkt_offset=off.ctypes.data, dst=col("dst", np.int32),
                          verdict=col("verdict", np.uint8), rssi=rssi, sinr=col("sinr", np.float64),
                          pkt_rssi=None if rssi is not None else col("pkt_rssi", np.float64))

    @staticmethod
    def unicast_from_result(result, src, n_nodes, want, fields=None):
        """rm_unicast_from_result (pure host function): the same answer from one tick's host result -- a _lib.HostResult, or
        anything with pkt_offset, dst, verdict and rssi or pkt_rssi (sinr optional), e.g. what tick_flush_view returns;
        src: the packets' sources (None: every packet sent)"""
        keep = []
        r = Engine._host_result(result, keep)
        want = np.ascontiguousarray(want, dtype=np.int32).reshape(-1)
        assert len(want) == r.n_packets
        if src is not None:
            src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
            assert len(src) == r.n_packets
        out, arrs = Engine._unicast_host_out(len(want), fields)
        check(_lib.lib().rm_unicast_from_result(C.byref(r), _ptr(src), n_nodes, want.ctypes.data, C.byref(out)))
        return arrs

    # -- receiver listening schedules: duty-cycled radios on the device
    @staticmethod
    def _listen_table(sched):
        """schedules as a contiguous LISTEN_SCHEDULE_DTYPE array: a structured array, or rows of (period_us, on_us, phase_us)"""
        a = np.asarray(sched)
        if a.dtype != _lib.LISTEN_SCHEDULE_DTYPE:
            rows = np.ascontiguousarray(a, dtype=np.int64).reshape(-1, 3)
            a = rows.view(_lib.LISTEN_SCHEDULE_DTYPE).reshape(-1)
        return np.ascontiguousarray(a.reshape(-1))

    def listen_set(self, sched, nodes=None):
        """rm_listen_set: sched for all nodes in node order, or for the listed nodes in list order (the last entry of a node wins);
        switches the feature on"""
        tbl = self._listen_table(sched)
        ptr, n, _idx = self._node_list(nodes)
        if nodes is not None and n != tbl.shape[0]:
            raise ValueError("one schedule per listed node")
        check(self._L.rm_listen_set(self._h, ptr, tbl.shape[0], tbl.ctypes.data))

    def listen_get(self, nodes=None):
        """rm_listen_get: structured array of LISTEN_SCHEDULE_DTYPE (the listed nodes in list order, or all in node order)"""
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=_lib.LISTEN_SCHEDULE_DTYPE)
        check(self._L.rm_listen_get(self._h, ptr, n, out.ctypes.data))
        return out

    def listen_clear(self):
        check(self._L.rm_listen_clear(self._h))

    def listen_enabled(self):
        return bool(self._L.rm_listen_enabled(self._h))

    def listen_missed(self, nodes=None):
        """rm_listen_missed_read: uint64 per node (the listed nodes in list order, or all in node order)"""
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=np.uint64)
        check(self._L.rm_listen_missed_read(self._h, ptr, n, out.ctypes.data))
        return out

    def listen_missed_reset(self):
        check(self._L.rm_listen_missed_reset(self._h))

    def listen_device(self):
        """rm_listen_device: (device pointer of the schedules [n_nodes] of 24-byte records, device pointer of missed [n_nodes] uint64)"""
        sch, mis = C.c_void_p(), C.c_void_p()
        check(self._L.rm_listen_device(self._h, C.byref(sch), C.byref(mis)))
        return sch.value, mis.value

    @staticmethod
    def listen_at(sched, t):
        """rm_listen_at (pure host): 1 / 0, or RM_ERR_INVALID for a bad record; sched = (period_us, on_us, phase_us)"""
        s = _lib.ListenSchedule(*[int(v) for v in sched])
        return int(_lib.lib().rm_listen_at(C.byref(s), int(t)))

    # -- watched-link statistics: per-link counters on the device
    def linkstats_enable(self, K):
        """rm_linkstats_enable: K = 1, 2, 4 or 8 slots of watched peers per node (all empty); 0 switches the feature off"""
        check(self._L.rm_linkstats_enable(self._h, int(K)))

    def linkstats_enabled(self):
        """rm_linkstats_enabled: K, or 0 while the feature is off"""
        return int(self._L.rm_linkstats_enabled(self._h))

    def _linkstats_rows(self, nodes):
        """(K, index array or None, rows) of a list call"""
        _, n, idx = self._node_list(nodes)
        return self.linkstats_enabled(), idx, n

    def linkstats_watch(self, peers, nodes=None):
        """rm_linkstats_watch: peers [n][K] (-1: an empty slot) for all nodes in node order, or for the listed nodes; a slot whose
        peer changes starts from a cleared entry, every other slot keeps its own"""
        K, idx, _ = self._linkstats_rows(nodes)
        rows = np.ascontiguousarray(peers, dtype=np.int32).reshape(-1, max(K, 1))
        if idx is not None and idx.shape[0] != rows.shape[0]:
            raise ValueError("one row of peers per listed node")
        check(self._L.rm_linkstats_watch(self._h, None if idx is None else idx.ctypes.data, rows.shape[0], rows.ctypes.data))

    def linkstats_peers(self, nodes=None):
        """rm_linkstats_peers_get: int32 [n][K] (the listed nodes in list order, or all in node order)"""
        K, idx, n = self._linkstats_rows(nodes)
        out = np.full((n, max(K, 1)), -1, dtype=np.int32)
        check(self._L.rm_linkstats_peers_get(self._h, None if idx is None else idx.ctypes.data, n, out.ctypes.data))
        return out

    def linkstats_read(self, nodes=None):
        """rm_linkstats_read: (structured array [n][K] of LINK_STATS_DTYPE -- the listed nodes in list order, or all in node order
        --, {"ticks_counted", "ticks_skipped"})"""
        K, idx, n = self._linkstats_rows(nodes)
        tot = _lib.StatsTotals()
        out = np.zeros((n, max(K, 1)), dtype=_lib.LINK_STATS_DTYPE)
        check(self._L.rm_linkstats_read(self._h, None if idx is None else idx.ctypes.data, n, out.ctypes.data, C.byref(tot)))
        return out, {"ticks_counted": int(tot.ticks_counted), "ticks_skipped": int(tot.ticks_skipped)}

    def linkstats_reset(self):
        check(self._L.rm_linkstats_reset(self._h))

    def linkstats_device(self):
        """rm_linkstats_device: device pointers of (peer [n_nodes][K] int32, entries [n_nodes][K] of 48-byte records, totals)"""
        peer, tbl, tot = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self._L.rm_linkstats_device(self._h, C.byref(peer), C.byref(tbl), C.byref(tot)))
        return peer.value, tbl.value, tot.value

    @staticmethod
    def linkstats_q8(x):
        """rm_linkstats_q8 (pure host): a dB value in 1/256 dB, rounded half up; 0 for NaN, an infinity or |x| >= 2^31"""
        return int(_lib.lib().rm_linkstats_q8(float(x)))

    @staticmethod
    def linkstats_validate(n_nodes, K, peers, nodes=None):
        """rm_linkstats_validate (pure host): the return code of the validation rm_linkstats_watch runs (0: accepted)"""
        rows = np.ascontiguousarray(peers, dtype=np.int32).reshape(-1)
        n = rows.shape[0] // K if K > 0 else rows.shape[0]
        idx = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        return int(_lib.lib().rm_linkstats_validate(int(n_nodes), int(K), None if idx is None else idx.ctypes.data,
                                                   n if idx is None else idx.shape[0], rows.ctypes.data))

    # -- traffic schedules: periodic sources generated on the device
    @staticmethod
    def _traffic_table(sched):
        """schedules as a contiguous TRAFFIC_SCHEDULE_DTYPE array: a structured array, or 2-D rows of (period_us, phase_us,
        jitter_us[, reserved]); a 1-D sequence of three or four values is ONE record, an empty one is no record"""
        a = np.asarray(sched)
        if a.dtype != _lib.TRAFFIC_SCHEDULE_DTYPE:
            rows = np.asarray(a, dtype=np.int64)
            if rows.ndim == 1:
                if rows.shape[0] not in (0, 3, 4):
                    raise ValueError("a schedule is (period_us, phase_us, jitter_us); several schedules are 2-D rows")
                rows = rows.reshape(-1, rows.shape[0] or 3)
            rows = rows.reshape(-1, rows.shape[-1])
            if rows.shape[1] == 3:
                rows = np.concatenate([rows, np.zeros((rows.shape[0], 1), dtype=np.int64)], axis=1)
            if rows.shape[1] != 4:
                raise ValueError("a schedule is (period_us, phase_us, jitter_us)")
            a = np.ascontiguousarray(rows).view(_lib.TRAFFIC_SCHEDULE_DTYPE).reshape(-1)
        return np.ascontiguousarray(a.reshape(-1))

    def traffic_set(self, sched, nodes=None):
        """rm_traffic_set: sched for all nodes in node order, or for the listed nodes in list order (the last entry of a node wins);
        switches the feature on"""
        tbl = self._traffic_table(sched)
        ptr, n, _idx = self._node_list(nodes)
        if nodes is not None and n != tbl.shape[0]:
            raise ValueError("one schedule per listed node")
        check(self._L.rm_traffic_set(self._h, ptr, tbl.shape[0], tbl.ctypes.data))

    def traffic_get(self, nodes=None):
        """rm_traffic_get: structured array of TRAFFIC_SCHEDULE_DTYPE (the listed nodes in list order, or all in node order)"""
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=_lib.TRAFFIC_SCHEDULE_DTYPE)
        check(self._L.rm_traffic_get(self._h, ptr, n, out.ctypes.data))
        return out

    def traffic_clear(self):
        check(self._L.rm_traffic_clear(self._h))

    def traffic_enabled(self):
        return bool(self._L.rm_traffic_enabled(self._h))

    def traffic_device(self):
        """rm_traffic_device: device pointer of the schedules, [n_nodes] of 32-byte records"""
        p = C.c_void_p()
        check(self._L.rm_traffic_device(self._h, C.byref(p)))
        return p.value

    @staticmethod
    def _traffic_windows(win_lo, win_hi):
        lo, hi = np.ascontiguousarray(win_lo, dtype=np.int64).reshape(-1), np.ascontiguousarray(win_hi, dtype=np.int64).reshape(-1)
        if lo.shape != hi.shape:
            raise ValueError("one win_hi per win_lo")
        return lo, hi

    def traffic_generate(self, seed, win_lo, win_hi, cap):
        """rm_traffic_generate: -> (rows int32[n_ticks][cap], ascending node indices padded with -1; count int32[n_ticks], the true
        number of sources per window; totals {packets, coalesced, truncated})"""
        lo, hi = self._traffic_windows(win_lo, win_hi)
        rows = np.empty((lo.shape[0], max(int(cap), 0)), dtype=np.int32)
        count = np.empty(lo.shape[0], dtype=np.int32)
        tot = _lib.TrafficTotals()
        check(self._L.rm_traffic_generate(self._h, int(seed) & (2 ** 64 - 1), lo.shape[0], lo.ctypes.data, hi.ctypes.data, int(cap),
                                          rows.ctypes.data, count.ctypes.data, C.byref(tot)))
        return rows, count, {"packets": tot.packets, "coalesced": tot.coalesced, "truncated": tot.truncated}

    def traffic_generate_device(self, seed, win_lo, win_hi, cap, dev_src_ptr, dev_count_ptr, dev_totals_ptr=None):
        """The raw form: device outputs (int32[n_ticks][cap], int32[n_ticks], one rm_traffic_totals or None), enqueued on the
        context's stream without waiting; row b is a ready device source list at dev_src_ptr + 4 * b * cap."""
        lo, hi = self._traffic_windows(win_lo, win_hi)
        check(self._L.rm_traffic_generate_device(self._h, int(seed) & (2 ** 64 - 1), lo.shape[0], lo.ctypes.data, hi.ctypes.data, int(cap),
                                                 dev_src_ptr, dev_count_ptr, dev_totals_ptr))

    @staticmethod
    def traffic_due(sched, seed, node, k):
        """rm_traffic_due (pure host): the due time of packet k of `node`, None for period 0; sched = (period_us, phase_us, jitter_us).
        Raises RadioMediumError for what the rule refuses."""
        s = _lib.TrafficSchedule(*[int(v) for v in sched])
        due = C.c_int64()
        rc = int(_lib.lib().rm_traffic_due(C.byref(s), int(seed) & (2 ** 64 - 1), int(node), int(k), C.byref(due)))
        if rc < 0:
            raise _lib.RadioMediumError(rc, "rm_traffic_due: a bad record, node or packet number")
        return due.value if rc == 1 else None

    @staticmethod
    def traffic_validate(n_nodes, sched, nodes=None):
        """rm_traffic_validate (pure host): the return code of the validation rm_traffic_set runs (0: accepted)"""
        tbl = Engine._traffic_table(sched)
        idx = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        return int(_lib.lib().rm_traffic_validate(int(n_nodes), None if idx is None else idx.ctypes.data,
                                                  tbl.shape[0] if idx is None else idx.shape[0], tbl.ctypes.data))

    # -- neighbour query: each node's K strongest potential links
    NB_HEARD_BY, NB_HEARS, NB_MAX_K = _lib.NB_HEARD_BY, _lib.NB_HEARS, _lib.NB_MAX_K

    @staticmethod
    def _neighbors_out(n, K, fields):
        """host arrays for n rows -> {name: array}; fields: the optional outputs asked for (None: rssi and degree)"""
        out = {"peer": np.empty((n, max(int(K), 0)), dtype=np.int32)}
        if fields is None or "rssi" in fields:
            out["rssi"] = np.empty((n, max(int(K), 0)), dtype=np.float64)
        if fields is None or "degree" in fields:
            out["degree"] = np.empty(n, dtype=np.int32)
        return out

    def neighbors(self, direction, K, nodes=None, fields=None):
        """rm_neighbors_query: the first K potential links of the listed nodes (None: all nodes in node order), ranked by rssi
        descending, then by node index -> {"peer": int32[n][K] padded with -1, "rssi": float64[n][K] (NaN beside a -1), "degree":
        int32[n], all potential links}.  direction NB_HEARD_BY: the node transmits; NB_HEARS: it receives."""
        idx = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        n = max(int(self._L.rm_node_count(self._h)), 0) if idx is None else idx.shape[0]
        out = self._neighbors_out(n, K, fields)
        check(self._L.rm_neighbors_query(self._h, int(direction), int(K), _ptr(idx), n, out["peer"].ctypes.data, _ptr(out.get("rssi")),
                                         _ptr(out.get("degree"))))
        return out

    def neighbors_device(self, direction, K, dev_peer_ptr, dev_rssi_ptr=None, dev_degree_ptr=None, dev_nodes_ptr=None, n=None):
        """rm_neighbors_query_device: the raw form -- device outputs (int32[n][K], float64[n][K] or None, int32[n] or None), the list
        in device memory (None: all nodes, n the node count); enqueued on the context's stream without waiting"""
        if n is None:
            if dev_nodes_ptr is not None:
                raise ValueError("a device list needs its length")
            n = int(self._L.rm_node_count(self._h))
        check(self._L.rm_neighbors_query_device(self._h, int(direction), int(K), dev_nodes_ptr, int(n), dev_peer_ptr, dev_rssi_ptr, dev_degree_ptr))

    @staticmethod
    def neighbors_from_result(result, K, n_pkt=None, fields=None):
        """rm_neighbors_from_result (pure host function): the same order over the heard links of each packet of one tick's host
        result -- a _lib.HostResult, or anything with count, pkt_offset, dst and rssi or pkt_rssi, e.g. what tick_flush_view returns"""
        keep = []
        if isinstance(result, HostResult):
            r = result
        else:
            def col(name, dt):
                a = getattr(result, name, None)
                if a is None:
                    return None
                a = np.ascontiguousarray(a, dtype=dt)
                keep.append(a)
                return a.ctypes.data
            off = np.ascontiguousarray(result.pkt_offset, dtype=np.uint32)
            keep.append(off)
            rssi = col("rssi", np.float64)
            r = HostResult(count=int(result.count), n_packets=len(off) - 1, pkt_offset=off.ctypes.data, dst=col("dst", np.int32),
                           rssi=rssi, pkt_rssi=None if rssi is not None else col("pkt_rssi", np.float64))
        n = int(r.n_packets) if n_pkt is None else int(n_pkt)
        out = Engine._neighbors_out(max(n, 0), K, fields)
        check(_lib.lib().rm_neighbors_from_result(C.byref(r), n, int(K), out["peer"].ctypes.data, _ptr(out.get("rssi")), _ptr(out.get("degree"))))
        return out

    # -- hop query: hop count and best parent toward a set of roots
    @staticmethod
    def _hops_out(n, fields):
        """host arrays for n nodes -> ({name: array}, the rm_hops_out over them); fields: the optional outputs asked for (None:
        all of parent, rssi, children)"""
        out = {name: np.empty(n, dtype=dt) for name, dt in _lib.HOPS_FIELDS if name == "hop" or fields is None or name in fields}
        return out, _lib.HopsOut(**{name: a.ctypes.data for name, a in out.items()})

    @staticmethod
    def _hops_totals(tot):
        return {"reached": int(tot.reached), "max_hop": int(tot.max_hop), "roots": int(tot.roots)}

    def hops(self, direction, roots, min_rssi_dbm=-np.inf, fields=None):
        """rm_hops_query: breadth-first levels from the roots over the potential links with rssi >= min_rssi_dbm ->
        ({"hop": int32[n] (-1: not reached), "parent": int32[n], "rssi": float64[n] (NaN beside a -1), "children": int32[n]},
        {"reached", "max_hop", "roots"}).  direction is the link between a node and its parent, seen from the node: NB_HEARD_BY a
        collection tree, NB_HEARS a dissemination tree."""
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        out, st = self._hops_out(max(int(self._L.rm_node_count(self._h)), 0), fields)
        tot = _lib.HopsTotals()
        check(self._L.rm_hops_query(self._h, int(direction), float(min_rssi_dbm), _ptr(idx), idx.shape[0], C.byref(st), C.byref(tot)))
        return out, self._hops_totals(tot)

    def hops_device(self, direction, dev_roots_ptr, n_roots, dev_hop_ptr, dev_parent_ptr=None, dev_rssi_ptr=None, dev_children_ptr=None,
                    min_rssi_dbm=-np.inf):
        """rm_hops_query_device: the raw form -- roots and outputs (int32[n], int32[n] or None, float64[n] or None, int32[n] or
        None) in device memory; waits once per level, complete on return -> {"reached", "max_hop", "roots"}"""
        st = _lib.HopsOut(hop=dev_hop_ptr, parent=dev_parent_ptr, rssi=dev_rssi_ptr, children=dev_children_ptr)
        tot = _lib.HopsTotals()
        check(self._L.rm_hops_query_device(self._h, int(direction), float(min_rssi_dbm), dev_roots_ptr, int(n_roots), C.byref(st), C.byref(tot)))
        return self._hops_totals(tot)

    def hops_next_device(self, dev_parent_ptr, dev_src_ptr, n, dev_want_ptr):
        """rm_hops_next_device: want[i] = parent[src[i]] (-1 for a source outside the table), all device memory -- the want list
        of unicast_query_device over source rows; enqueued without waiting"""
        check(self._L.rm_hops_next_device(self._h, dev_parent_ptr, dev_src_ptr, int(n), dev_want_ptr))

    @staticmethod
    def hops_from_links(n_nodes, node, far, rssi, roots, min_rssi_dbm=-np.inf, fields=None):
        """rm_hops_from_links (pure host function): the same rule over an explicit list of candidate links -- far[i] may be
        node[i]'s parent with rssi[i] -> what hops returns"""
        node = np.ascontiguousarray(node, dtype=np.int32).reshape(-1)
        far = np.ascontiguousarray(far, dtype=np.int32).reshape(-1)
        rssi = np.ascontiguousarray(rssi, dtype=np.float64).reshape(-1)
        if not (node.shape == far.shape == rssi.shape):
            raise ValueError("node, far and rssi have one entry per link")
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        out, st = Engine._hops_out(max(int(n_nodes), 0), fields)
        tot = _lib.HopsTotals()
        check(_lib.lib().rm_hops_from_links(int(n_nodes), node.shape[0], _ptr(node), _ptr(far), _ptr(rssi), float(min_rssi_dbm), _ptr(idx),
                                            idx.shape[0], C.byref(st), C.byref(tot)))
        return out, Engine._hops_totals(tot)

    # -- route query: minimum-ETX routes toward a set of roots
    @staticmethod
    def routes_params(direction=_lib.NB_HEARD_BY, kind=_lib.EM_OQPSK_250K, us_per_bit=4.0, air_us=4064, min_rssi_dbm=-np.inf,
                      max_link_cost=1024, reserved=0):
        """an rm_routes_params"""
        return _lib.RoutesParams(direction=int(direction), kind=int(kind), us_per_bit=float(us_per_bit), air_us=int(air_us),
                                 min_rssi_dbm=float(min_rssi_dbm), max_link_cost=int(max_link_cost), reserved=int(reserved))

    @staticmethod
    def _routes_out(n, fields):
        out = {name: np.empty(n, dtype=dt) for name, dt in _lib.ROUTES_FIELDS if name == "cost" or fields is None or name in fields}
        return out, _lib.RoutesOut(**{name: a.ctypes.data for name, a in out.items()})

    @staticmethod
    def _routes_totals(tot):
        return {"reached": int(tot.reached), "roots": int(tot.roots), "max_cost": int(tot.max_cost)}

    def routes(self, params, roots, fields=None):
        """rm_routes_query: least path cost (ETX in units of 1/128) toward the roots over the potential links and the parent on
        such a path -> ({"cost": uint64[n] (ROUTE_UNREACHED: not reached), "parent": int32[n], "rssi": float64[n] (NaN beside a
        -1), "link_cost": uint32[n], "children": int32[n]}, {"reached", "roots", "max_cost"}).  params: routes_params(...)"""
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        out, st = self._routes_out(max(int(self._L.rm_node_count(self._h)), 0), fields)
        tot = _lib.RoutesTotals()
        check(self._L.rm_routes_query(self._h, C.byref(params), _ptr(idx), idx.shape[0], C.byref(st), C.byref(tot)))
        return out, self._routes_totals(tot)

    def routes_device(self, params, dev_roots_ptr, n_roots, dev_cost_ptr, dev_parent_ptr=None, dev_rssi_ptr=None, dev_link_cost_ptr=None,
                      dev_children_ptr=None):
        """rm_routes_query_device: the raw form -- roots and outputs (uint64[n], int32[n], float64[n], uint32[n], int32[n]; all but
        the first may be None) in device memory; waits once per round, complete on return -> {"reached", "roots", "max_cost"}"""
        st = _lib.RoutesOut(cost=dev_cost_ptr, parent=dev_parent_ptr, rssi=dev_rssi_ptr, link_cost=dev_link_cost_ptr, children=dev_children_ptr)
        tot = _lib.RoutesTotals()
        check(self._L.rm_routes_query_device(self._h, C.byref(params), dev_roots_ptr, int(n_roots), C.byref(st), C.byref(tot)))
        return self._routes_totals(tot)

    def routes_last_work(self):
        """rm_routes_last_work: (relaxation rounds, frontier entries walked in all) of the last completed route query"""
        rounds, entries = C.c_int32(0), C.c_uint64(0)
        check(self._L.rm_routes_last_work(self._h, C.byref(rounds), C.byref(entries)))
        return int(rounds.value), int(entries.value)

    @staticmethod
    def route_link_cost(params, noise_dbm, rssi):
        """rm_routes_link_cost (pure host function): the cost of a link of this rssi, or None when it does not count"""
        c = C.c_uint32(0)
        return int(c.value) if _lib.lib().rm_routes_link_cost(C.byref(params), float(noise_dbm), float(rssi), C.byref(c)) else None

    @staticmethod
    def routes_from_links(n_nodes, node, far, rssi, params, noise_dbm, roots, fields=None):
        """rm_routes_from_links (pure host function): the same rule over an explicit list of candidate links -- far[i] may be
        node[i]'s parent with rssi[i] -> what routes returns"""
        node = np.ascontiguousarray(node, dtype=np.int32).reshape(-1)
        far = np.ascontiguousarray(far, dtype=np.int32).reshape(-1)
        rssi = np.ascontiguousarray(rssi, dtype=np.float64).reshape(-1)
        if not (node.shape == far.shape == rssi.shape):
            raise ValueError("node, far and rssi have one entry per link")
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        out, st = Engine._routes_out(max(int(n_nodes), 0), fields)
        tot = _lib.RoutesTotals()
        check(_lib.lib().rm_routes_from_links(int(n_nodes), node.shape[0], _ptr(node), _ptr(far), _ptr(rssi), C.byref(params), float(noise_dbm),
                                              _ptr(idx), idx.shape[0], C.byref(st), C.byref(tot)))
        return out, Engine._routes_totals(tot)

    # -- measured-route query: minimum-ETX routes over watched-link statistics
    @staticmethod
    def etx_params(**kw):
        """rm_etx_defaults with the given fields replaced: mode, min_heard, max_link_cost, hysteresis (and the reserved ones)"""
        p = _lib.EtxParams()
        _lib.lib().rm_etx_defaults(C.byref(p))
        for k, v in kw.items():
            if k not in dict(_lib.EtxParams._fields_):
                raise TypeError("rm_etx_params has no field " + k)
            setattr(p, k, int(v))
        return p

    @staticmethod
    def etx_validate(params):
        """rm_etx_validate (pure host): 0 when the query would accept the parameters"""
        return int(_lib.lib().rm_etx_validate(C.byref(params)))

    @staticmethod
    def _etx_out(n, fields):
        out = {name: np.empty(n, dtype=dt) for name, dt in _lib.ETX_FIELDS if name == "cost" or fields is None or name in fields}
        return out, _lib.EtxOut(**{name: a.ctypes.data for name, a in out.items()})

    @staticmethod
    def _etx_totals(tot):
        return {k: int(getattr(tot, k)) for k in ("reached", "roots", "kept", "switched", "lost", "max_cost")}

    @staticmethod
    def _etx_tables(tables, keep):
        """(peer [n][K], stats [n][K] of LINK_STATS_DTYPE) as host arrays -> an rm_etx_tables over contiguous copies (held in keep)"""
        peer = np.ascontiguousarray(tables[0], dtype=np.int32)
        stats = np.ascontiguousarray(tables[1], dtype=_lib.LINK_STATS_DTYPE)
        if peer.ndim != 2 or stats.shape != peer.shape:
            raise ValueError("peer and stats are [n_nodes][K]")
        keep += [peer, stats]
        return _lib.EtxTables(peer=peer.ctypes.data, stats=stats.ctypes.data, K=peer.shape[1], reserved=0)

    def etx_routes(self, params, roots, tables=None, cur=None, fields=None):
        """rm_etx_query: least measured-ETX path cost (units of 1/128) toward the roots over a watch table and the parent on it,
        the current parent kept within params.hysteresis -> ({"cost": uint64[n] (ROUTE_UNREACHED: not reached), "parent":
        int32[n], "slot": int32[n], "link_cost": uint32[n], "children": int32[n]}, {"reached", "roots", "kept", "switched", "lost",
        "max_cost"}).  tables: None (the context's own watched-link tables) or (peer [n][K], stats [n][K]); cur: None or the
        current parents int32[n]; params: etx_params(...)"""
        keep = []
        n = max(int(self._L.rm_node_count(self._h)), 0)
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        t = None if tables is None else self._etx_tables(tables, keep)
        if t is not None and keep[0].shape[0] != n:
            raise ValueError("one row of the tables per node")
        c = None if cur is None else np.ascontiguousarray(cur, dtype=np.int32).reshape(-1)
        if c is not None and c.shape[0] != n:
            raise ValueError("one current parent per node")
        out, st = self._etx_out(n, fields)
        tot = _lib.EtxTotals()
        check(self._L.rm_etx_query(self._h, C.byref(params), None if t is None else C.byref(t), _ptr(idx), idx.shape[0], _ptr(c), C.byref(st),
                                   C.byref(tot)))
        return out, self._etx_totals(tot)

    def etx_routes_device(self, params, dev_roots_ptr, n_roots, dev_cost_ptr, dev_parent_ptr=None, dev_slot_ptr=None, dev_link_cost_ptr=None,
                          dev_children_ptr=None, dev_cur_ptr=None, dev_tables=None):
        """rm_etx_query_device: the raw form -- roots, cur (or None), outputs (uint64[n], int32[n], int32[n], uint32[n], int32[n];
        all but the first may be None) and dev_tables (None: the context's own, or (peer pointer, stats pointer, K)) in device
        memory; dev_cur_ptr may be dev_parent_ptr; waits once per round, complete on return -> the totals"""
        st = _lib.EtxOut(cost=dev_cost_ptr, parent=dev_parent_ptr, slot=dev_slot_ptr, link_cost=dev_link_cost_ptr, children=dev_children_ptr)
        t = None if dev_tables is None else _lib.EtxTables(peer=dev_tables[0], stats=dev_tables[1], K=int(dev_tables[2]), reserved=0)
        tot = _lib.EtxTotals()
        check(self._L.rm_etx_query_device(self._h, C.byref(params), None if t is None else C.byref(t), dev_roots_ptr, int(n_roots), dev_cur_ptr,
                                          C.byref(st), C.byref(tot)))
        return self._etx_totals(tot)

    def etx_last_work(self):
        """rm_etx_last_work: (relaxation rounds, nodes examined in all) of the last completed measured-route query"""
        rounds, examined = C.c_int32(0), C.c_uint64(0)
        check(self._L.rm_etx_last_work(self._h, C.byref(rounds), C.byref(examined)))
        return int(rounds.value), int(examined.value)

    @staticmethod
    def etx_link_cost(params, heard, delivered):
        """rm_etx_link_cost (pure host function): the inbound cost of an entry with these counters, or None when it does not count"""
        c = C.c_uint32(0)
        return int(c.value) if _lib.lib().rm_etx_link_cost(C.byref(params), int(heard), int(delivered), C.byref(c)) else None

    @staticmethod
    def etx_combine(c_in, c_rev):
        """rm_etx_combine (pure host function): RM_ETX_BOTH's cost of two inbound costs"""
        return int(_lib.lib().rm_etx_combine(int(c_in), int(c_rev)))

    @staticmethod
    def etx_from_tables(tables, params, roots, cur=None, fields=None):
        """rm_etx_from_tables (pure host function, a heap Dijkstra): the same rule over (peer [n][K], stats [n][K]) -> what
        etx_routes returns"""
        keep = []
        t = Engine._etx_tables(tables, keep)
        n = keep[0].shape[0]
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        c = None if cur is None else np.ascontiguousarray(cur, dtype=np.int32).reshape(-1)
        if c is not None and c.shape[0] != n:
            raise ValueError("one current parent per node")
        out, st = Engine._etx_out(n, fields)
        tot = _lib.EtxTotals()
        check(_lib.lib().rm_etx_from_tables(n, C.byref(t), C.byref(params), _ptr(idx), idx.shape[0], _ptr(c), C.byref(st), C.byref(tot)))
        return out, Engine._etx_totals(tot)

    def linkstats_watch_device(self, dev_peers_ptr, dev_nodes_ptr=None, n=None):
        """rm_linkstats_watch_device: rm_linkstats_watch with rows (int32[n][K] of the enabled K) and list in device memory (None: all
        nodes) -- e.g. the peer block of neighbors_device(NB_HEARS, K); validated on the device, waited for"""
        if n is None:
            if dev_nodes_ptr is not None:
                raise ValueError("a device list needs its length")
            n = int(self._L.rm_node_count(self._h))
        check(self._L.rm_linkstats_watch_device(self._h, dev_nodes_ptr, int(n), dev_peers_ptr))

    def linkstats_stage_device(self):
        """rm_linkstats_stage_device: device pointer of a block the context owns with room for n_nodes x K rows (a caller without a
        device allocator chains neighbors_device -> linkstats_watch_device through it)"""
        p = C.c_void_p()
        check(self._L.rm_linkstats_stage_device(self._h, C.byref(p)))
        return p.value

    # -- forwarding queues: multi-hop packet relay on the device
    @staticmethod
    def fwd_params(**kw):
        """rm_fwd_defaults with the given fields replaced: queue_slots, max_retries, min_be, max_be, max_hops, backoff_unit_us, seed"""
        p = _lib.FwdParams()
        _lib.lib().rm_fwd_defaults(C.byref(p))
        for k, v in kw.items():
            if k not in dict(_lib.FwdParams._fields_):
                raise TypeError("rm_fwd_params has no field " + k)
            setattr(p, k, int(v) & (2 ** 64 - 1) if k == "seed" else int(v))
        return p

    @staticmethod
    def fwd_validate(params):
        """rm_fwd_validate (pure host): the return code of the validation rm_fwd_enable runs (0: accepted)"""
        return int(_lib.lib().rm_fwd_validate(C.byref(params)))

    @staticmethod
    def fwd_backoff(params, node, start_us, tries):
        """rm_fwd_backoff (pure host): the delay in us behind a frame's end after the node's `tries`-th failed attempt in a row"""
        d = C.c_int64()
        check(_lib.lib().rm_fwd_backoff(C.byref(params), int(node), int(start_us), int(tries), C.byref(d)))
        return d.value

    def fwd_enable(self, params=None, **kw):
        """rm_fwd_enable: the queues made (again: cleared, every next -1) with `params` or fwd_params(**kw)"""
        p = params if params is not None else self.fwd_params(**kw)
        check(self._L.rm_fwd_enable(self._h, C.byref(p)))

    def fwd_get_params(self):
        """rm_fwd_get_params: the enabled parameters"""
        p = _lib.FwdParams()
        check(self._L.rm_fwd_get_params(self._h, C.byref(p)))
        return p

    def fwd_disable(self):
        check(self._L.rm_fwd_disable(self._h))

    def fwd_enabled(self):
        return bool(self._L.rm_fwd_enabled(self._h))

    def fwd_reset(self):
        """rm_fwd_reset: counters, totals and queues cleared; next and the parameters kept"""
        check(self._L.rm_fwd_reset(self._h))

    def fwd_set_next(self, parent, roots, time_us):
        """rm_fwd_set_next: next = parent (int32[n_nodes]; outside the table or itself: no route), the roots sinks; queues settled"""
        par = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        if par.shape[0] != max(int(self._L.rm_node_count(self._h)), 0):
            raise ValueError("one parent per node")
        idx = np.ascontiguousarray(roots, dtype=np.int32).reshape(-1)
        check(self._L.rm_fwd_set_next(self._h, par.ctypes.data, _ptr(idx) if idx.shape[0] else None, idx.shape[0], int(time_us)))

    def fwd_set_next_device(self, dev_parent_ptr, dev_roots_ptr, n_roots, time_us):
        """The raw form: a hop or route query's parent array and root list as they lie in device memory; not waited for"""
        check(self._L.rm_fwd_set_next_device(self._h, dev_parent_ptr, dev_roots_ptr, int(n_roots), int(time_us)))

    def fwd_inject(self, src, time_us):
        """rm_fwd_inject: one new packet per entry at its node (negative: padding)"""
        idx = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        check(self._L.rm_fwd_inject(self._h, _ptr(idx) if idx.shape[0] else None, idx.shape[0], int(time_us)))

    def fwd_inject_device(self, dev_src_ptr, n, time_us):
        check(self._L.rm_fwd_inject_device(self._h, dev_src_ptr, int(n), int(time_us)))

    def fwd_sources(self, time_us, cap):
        """rm_fwd_sources: -> (int32[cap], the nodes sendable at time_us ascending, padded with -1; their true number)"""
        out = np.empty(max(int(cap), 0), dtype=np.int32)
        count = C.c_int32()
        check(self._L.rm_fwd_sources(self._h, int(time_us), int(cap), out.ctypes.data if out.shape[0] else None, C.byref(count)))
        return out, count.value

    def fwd_sources_device(self, time_us, cap, dev_src_ptr, dev_count_ptr):
        """The raw form: int32[cap] and one int32 in device memory, a ready source list of the device ticks; not waited for"""
        check(self._L.rm_fwd_sources_device(self._h, int(time_us), int(cap), dev_src_ptr, dev_count_ptr))

    def fwd_advance(self, slot=0, cand=None):
        """rm_fwd_advance: result slot `slot` of the last evaluating call moves the queues; cand: the candidate list handed to that
        call (a gated tick), None: the frames' own sources"""
        if cand is None:
            check(self._L.rm_fwd_advance(self._h, int(slot), None, 0))
            return
        idx = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1)
        keep = idx if idx.shape[0] else np.zeros(1, dtype=np.int32)
        check(self._L.rm_fwd_advance(self._h, int(slot), keep.ctypes.data, idx.shape[0]))

    def fwd_advance_device(self, slot, dev_cand_ptr, n_cand):
        check(self._L.rm_fwd_advance_device(self._h, int(slot), dev_cand_ptr, int(n_cand)))

    def fwd_read(self, nodes=None):
        """rm_fwd_read: (structured array of FWD_NODE_DTYPE -- the listed nodes in list order, or all --, the totals as a dict)"""
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=_lib.FWD_NODE_DTYPE)
        tot = np.zeros(1, dtype=_lib.FWD_TOTALS_DTYPE)
        check(self._L.rm_fwd_read(self._h, ptr, n, out.ctypes.data if n else None, tot.ctypes.data))
        return out, {k: int(tot[k][0]) for k in tot.dtype.names}

    def fwd_queue_read(self, nodes=None):
        """rm_fwd_queue_read: (FWD_PACKET_DTYPE[n][queue_slots] in queue order, int32[n] the queues' lengths); queue_slots is
        the enabled parameters' (rm_fwd_get_params)"""
        q = int(self.fwd_get_params().queue_slots)
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros((n, q), dtype=_lib.FWD_PACKET_DTYPE)
        ln = np.zeros(n, dtype=np.int32)
        check(self._L.rm_fwd_queue_read(self._h, ptr, n, out.ctypes.data if n else None, ln.ctypes.data if n else None))
        return out, ln

    def fwd_device(self):
        """rm_fwd_device: device pointers (rows [n_nodes] of 128 bytes, packets [n_nodes][queue_slots] of 24 bytes, totals)"""
        a, b, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self._L.rm_fwd_device(self._h, C.byref(a), C.byref(b), C.byref(t)))
        return a.value, b.value, t.value

    # -- dissemination floods: Trickle-timed broadcast relay on the device
    @staticmethod
    def flood_params(**kw):
        """rm_flood_defaults with the given fields replaced: imin_us, doublings, max_intervals, redundancy, max_hops, seed"""
        p = _lib.FloodParams()
        _lib.lib().rm_flood_defaults(C.byref(p))
        for k, v in kw.items():
            if k not in dict(_lib.FloodParams._fields_):
                raise TypeError("rm_flood_params has no field " + k)
            setattr(p, k, int(v) & (2 ** 64 - 1) if k == "seed" else int(v))
        return p

    @staticmethod
    def flood_validate(params):
        """rm_flood_validate (pure host): the return code of the validation rm_flood_enable runs (0: accepted)"""
        return int(_lib.lib().rm_flood_validate(C.byref(params)))

    @staticmethod
    def flood_fire(params, node, first_us, m):
        """rm_flood_fire (pure host): (start_us, fire_us) of interval m of a node that got the data at first_us; (-1, -1): done"""
        s, f = C.c_int64(), C.c_int64()
        check(_lib.lib().rm_flood_fire(C.byref(params), int(node), int(first_us), int(m), C.byref(s), C.byref(f)))
        return s.value, f.value

    def flood_enable(self, params=None, **kw):
        """rm_flood_enable: the table made (again: cleared) with `params` or flood_params(**kw)"""
        p = params if params is not None else self.flood_params(**kw)
        check(self._L.rm_flood_enable(self._h, C.byref(p)))

    def flood_get_params(self):
        p = _lib.FloodParams()
        check(self._L.rm_flood_get_params(self._h, C.byref(p)))
        return p

    def flood_disable(self):
        check(self._L.rm_flood_disable(self._h))

    def flood_enabled(self):
        return bool(self._L.rm_flood_enabled(self._h))

    def flood_reset(self):
        """rm_flood_reset: nobody has the data, counters and totals zero; the parameters kept"""
        check(self._L.rm_flood_reset(self._h))

    def flood_seed(self, nodes, time_us):
        """rm_flood_seed: every listed node that lacks the data gets it at time_us (negative entries: padding)"""
        idx = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        check(self._L.rm_flood_seed(self._h, _ptr(idx) if idx.shape[0] else None, idx.shape[0], int(time_us)))

    def flood_seed_device(self, dev_nodes_ptr, n, time_us):
        check(self._L.rm_flood_seed_device(self._h, dev_nodes_ptr, int(n), int(time_us)))

    def flood_sources(self, time_us, cap):
        """rm_flood_sources: the suppression roll, then -> (int32[cap], the due nodes ascending, padded with -1; their true number)"""
        out = np.empty(max(int(cap), 0), dtype=np.int32)
        count = C.c_int32()
        check(self._L.rm_flood_sources(self._h, int(time_us), int(cap), out.ctypes.data if out.shape[0] else None, C.byref(count)))
        return out, count.value

    def flood_sources_device(self, time_us, cap, dev_src_ptr, dev_count_ptr):
        """The raw form: int32[cap] and one int32 in device memory, a ready source list of the device ticks; not waited for"""
        check(self._L.rm_flood_sources_device(self._h, int(time_us), int(cap), dev_src_ptr, dev_count_ptr))

    def flood_advance(self, slot=0, cand=None):
        """rm_flood_advance: result slot `slot` of the last evaluating call moves the flood; cand: the candidate list handed to that
        call (a gated tick), None: the frames' own sources"""
        if cand is None:
            check(self._L.rm_flood_advance(self._h, int(slot), None, 0))
            return
        idx = np.ascontiguousarray(cand, dtype=np.int32).reshape(-1)
        keep = idx if idx.shape[0] else np.zeros(1, dtype=np.int32)
        check(self._L.rm_flood_advance(self._h, int(slot), keep.ctypes.data, idx.shape[0]))

    def flood_advance_device(self, slot, dev_cand_ptr, n_cand):
        check(self._L.rm_flood_advance_device(self._h, int(slot), dev_cand_ptr, int(n_cand)))

    def flood_read(self, nodes=None):
        """rm_flood_read: (structured array of FLOOD_NODE_DTYPE -- the listed nodes in list order, or all --, the totals as a dict)"""
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=_lib.FLOOD_NODE_DTYPE)
        tot = np.zeros(1, dtype=_lib.FLOOD_TOTALS_DTYPE)
        check(self._L.rm_flood_read(self._h, ptr, n, out.ctypes.data if n else None, tot.ctypes.data))
        return out, {k: int(tot[k][0]) for k in tot.dtype.names}

    def flood_device(self):
        """rm_flood_device: device pointers (rows [n_nodes] of 64 bytes, totals)"""
        a, t = C.c_void_p(), C.c_void_p()
        check(self._L.rm_flood_device(self._h, C.byref(a), C.byref(t)))
        return a.value, t.value

    def flood_tree_device(self, dev_parent_ptr, dev_hop_ptr=None):
        """rm_flood_tree_device: parent (and hop) by node index into int32[n_nodes] arrays in device memory; not waited for"""
        check(self._L.rm_flood_tree_device(self._h, dev_parent_ptr, dev_hop_ptr))

    # -- neighbour tables: discover, evict and expire watched peers on the device
    @staticmethod
    def nbtable_params(**kw):
        """rm_nbtable_defaults with the given fields replaced: admit_rssi_dbm, timeout_us, min_heard, evict_cost, require_delivered"""
        p = _lib.NbTableParams()
        _lib.lib().rm_nbtable_defaults(C.byref(p))
        for k, v in kw.items():
            if k not in dict(_lib.NbTableParams._fields_):
                raise TypeError("rm_nbtable_params has no field " + k)
            setattr(p, k, v)
        return p

    @staticmethod
    def nbtable_validate(params):
        """rm_nbtable_validate (pure host): the return code of the validation rm_nbtable_enable runs (0: accepted)"""
        return int(_lib.lib().rm_nbtable_validate(C.byref(params)))

    def nbtable_enable(self, params=None, **kw):
        """rm_nbtable_enable: the counters made (again: cleared) with `params` or nbtable_params(**kw); needs linkstats_enable first"""
        p = params if params is not None else self.nbtable_params(**kw)
        check(self._L.rm_nbtable_enable(self._h, C.byref(p)))

    def nbtable_get_params(self):
        p = _lib.NbTableParams()
        check(self._L.rm_nbtable_get_params(self._h, C.byref(p)))
        return p

    def nbtable_disable(self):
        check(self._L.rm_nbtable_disable(self._h))

    def nbtable_enabled(self):
        return bool(self._L.rm_nbtable_enabled(self._h))

    def nbtable_reset(self):
        """rm_nbtable_reset: counters and totals zero; the watched-link statistics' tables are left alone"""
        check(self._L.rm_nbtable_reset(self._h))

    @staticmethod
    def _nbtable_pin(pin):
        return None if pin is None else np.ascontiguousarray(pin, dtype=np.int32).reshape(-1)

    def nbtable_update(self, slot, time_us, pin=None):
        """rm_nbtable_update: result slot `slot` of the last evaluating call admits at most one new peer per node; pin: int32
        [n_nodes] of protected peers (negative: none), e.g. the parents of a route query, or None"""
        p = self._nbtable_pin(pin)
        if p is not None and p.shape[0] != int(self._L.rm_node_count(self._h)):
            raise ValueError("one pin entry per node")
        check(self._L.rm_nbtable_update(self._h, int(slot), int(time_us), _ptr(p)))

    def nbtable_update_device(self, slot, time_us, dev_pin_ptr=None):
        """The raw form: pin as int32[n_nodes] in device memory (or None); enqueued on the context's stream, not waited for"""
        check(self._L.rm_nbtable_update_device(self._h, int(slot), int(time_us), dev_pin_ptr))

    def nbtable_expire(self, time_us, pin=None):
        """rm_nbtable_expire: every slot that is not empty, not pinned and stale at time_us becomes empty"""
        p = self._nbtable_pin(pin)
        if p is not None and p.shape[0] != int(self._L.rm_node_count(self._h)):
            raise ValueError("one pin entry per node")
        check(self._L.rm_nbtable_expire(self._h, int(time_us), _ptr(p)))

    def nbtable_expire_device(self, time_us, dev_pin_ptr=None):
        check(self._L.rm_nbtable_expire_device(self._h, int(time_us), dev_pin_ptr))

    def nbtable_read(self, nodes=None):
        """rm_nbtable_read: (structured array of NBTABLE_NODE_DTYPE -- the listed nodes in list order, or all --, the totals as a
        dict); the peers and entries themselves are linkstats_peers and linkstats_read"""
        ptr, n, _idx = self._node_list(nodes)
        out = np.zeros(n, dtype=_lib.NBTABLE_NODE_DTYPE)
        tot = np.zeros(1, dtype=_lib.NBTABLE_TOTALS_DTYPE)
        check(self._L.rm_nbtable_read(self._h, ptr, n, out.ctypes.data if n else None, tot.ctypes.data))
        return out, {k: int(tot[k][0]) for k in tot.dtype.names}

    def nbtable_device(self):
        """rm_nbtable_device: device pointers (rows [n_nodes] of 32 bytes, totals)"""
        a, t = C.c_void_p(), C.c_void_p()
        check(self._L.rm_nbtable_device(self._h, C.byref(a), C.byref(t)))
        return a.value, t.value

    @staticmethod
    def _nbtable_host_tables(peer, stats, node, totals):
        if peer.dtype != np.int32 or peer.ndim != 2 or not peer.flags.c_contiguous:
            raise ValueError("peer is a C-contiguous int32 [n_nodes][K] array, updated in place")
        if stats.dtype != _lib.LINK_STATS_DTYPE or stats.shape != peer.shape or not stats.flags.c_contiguous:
            raise ValueError("stats is a C-contiguous LINK_STATS_DTYPE [n_nodes][K] array, updated in place")
        n = peer.shape[0]
        if node is None:
            node = np.zeros(n, dtype=_lib.NBTABLE_NODE_DTYPE)
        if totals is None:
            totals = np.zeros(1, dtype=_lib.NBTABLE_TOTALS_DTYPE)
        if node.dtype != _lib.NBTABLE_NODE_DTYPE or node.shape != (n,) or totals.dtype != _lib.NBTABLE_TOTALS_DTYPE or totals.shape != (1,):
            raise ValueError("node is NBTABLE_NODE_DTYPE [n_nodes] and totals NBTABLE_TOTALS_DTYPE [1], both added to")
        return n, peer.shape[1], node, totals

    @staticmethod
    def nbtable_from_result(result, src, start_us, peer, stats, params, time_us, pin=None, node=None, totals=None):
        """rm_nbtable_from_result (pure host function): the update rule over one tick's host result (as unicast_from_result takes
        it) with the packets' src and start_us; peer (int32 [n][K]) and stats (LINK_STATS_DTYPE [n][K]) change in place, node and
        totals (made when None) are added to -> (node, totals)"""
        keep = []
        r = Engine._host_result(result, keep)
        n, K, node, totals = Engine._nbtable_host_tables(peer, stats, node, totals)
        src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        start = np.ascontiguousarray(start_us, dtype=np.int64).reshape(-1)
        assert len(src) == len(start) == r.n_packets
        p = Engine._nbtable_pin(pin)
        if p is not None and p.shape[0] != n:
            raise ValueError("one pin entry per node")
        check(_lib.lib().rm_nbtable_from_result(C.byref(r), _ptr(src), _ptr(start), n, K, peer.ctypes.data, stats.ctypes.data, C.byref(params),
                                                int(time_us), _ptr(p), node.ctypes.data, totals.ctypes.data))
        return node, totals

    @staticmethod
    def nbtable_expire_tables(peer, stats, params, time_us, pin=None, node=None, totals=None):
        """rm_nbtable_expire_tables (pure host function): the expire walk over host tables, in place -> (node, totals)"""
        n, K, node, totals = Engine._nbtable_host_tables(peer, stats, node, totals)
        p = Engine._nbtable_pin(pin)
        if p is not None and p.shape[0] != n:
            raise ValueError("one pin entry per node")
        check(_lib.lib().rm_nbtable_expire_tables(n, K, peer.ctypes.data, stats.ctypes.data, C.byref(params), int(time_us), _ptr(p),
                                                  node.ctypes.data, totals.ctypes.data))
        return node, totals

    # -- link estimator: EWMA ETX over counter windows and forwarding acks
    @staticmethod
    def linkest_params(**kw):
        """rm_linkest_defaults with the given fields replaced: beacon_window, data_window, beacon_alpha_q8, data_alpha_q8, max_etx"""
        p = _lib.LinkEstParams()
        _lib.lib().rm_linkest_defaults(C.byref(p))
        for k, v in kw.items():
            if k not in dict(_lib.LinkEstParams._fields_):
                raise TypeError("rm_linkest_params has no field " + k)
            setattr(p, k, int(v))
        return p

    @staticmethod
    def linkest_validate(params):
        """rm_linkest_validate (pure host): the return code of the validation rm_linkest_enable runs (0: accepted)"""
        return int(_lib.lib().rm_linkest_validate(C.byref(params)))

    def linkest_enable(self, K, params=None, **kw):
        """rm_linkest_enable: the tables made (again: in their after-enable state) for K slots per node with `params` or
        linkest_params(**kw)"""
        p = params if params is not None else self.linkest_params(**kw)
        check(self._L.rm_linkest_enable(self._h, int(K), C.byref(p)))

    def linkest_get_params(self):
        p = _lib.LinkEstParams()
        check(self._L.rm_linkest_get_params(self._h, C.byref(p)))
        return p

    def linkest_disable(self):
        check(self._L.rm_linkest_disable(self._h))

    def linkest_enabled(self):
        """K, or 0 while the feature is off"""
        return int(self._L.rm_linkest_enabled(self._h))

    def linkest_reset(self):
        """rm_linkest_reset: every table back to its after-enable state"""
        check(self._L.rm_linkest_reset(self._h))

    @staticmethod
    def _linkest_inputs(peer, stats, fwd, keep):
        """host arrays (peer int32 [n][K], stats LINK_STATS_DTYPE [n][K], fwd FWD_NODE_DTYPE [n] or None) -> rm_linkest_inputs"""
        peer = np.ascontiguousarray(peer, dtype=np.int32)
        stats = np.ascontiguousarray(stats, dtype=_lib.LINK_STATS_DTYPE)
        if peer.ndim != 2 or stats.shape != peer.shape:
            raise ValueError("peer and stats are [n_nodes][K]")
        keep += [peer, stats]
        f = None
        if fwd is not None:
            f = np.ascontiguousarray(fwd, dtype=_lib.FWD_NODE_DTYPE).reshape(-1)
            if f.shape[0] != peer.shape[0]:
                raise ValueError("one forwarding row per node")
            keep.append(f)
        return _lib.LinkEstInputs(peer=peer.ctypes.data, stats=stats.ctypes.data, fwd=_ptr(f), K=peer.shape[1], reserved=0)

    def linkest_fold(self, peer=None, stats=None, fwd=None):
        """rm_linkest_fold: one fold over the context's own tables (no arguments: E14's, and E19's while it is on) or over host
        arrays peer / stats [n_nodes][K] and fwd [n_nodes] (or None: no data step), uploaded first"""
        if peer is None and stats is None and fwd is None:
            check(self._L.rm_linkest_fold(self._h, None))
            return
        keep = []
        inp = self._linkest_inputs(peer, stats, fwd, keep)
        if keep[0].shape[0] != int(self._L.rm_node_count(self._h)):
            raise ValueError("one row of the inputs per node")
        check(self._L.rm_linkest_fold(self._h, C.byref(inp)))

    def linkest_fold_device(self, dev_inputs=None):
        """The raw form: None (the context's own tables) or (peer pointer, stats pointer, fwd pointer or None, K) in device memory;
        enqueued on the context's stream, not waited for"""
        if dev_inputs is None:
            check(self._L.rm_linkest_fold_device(self._h, None))
            return
        inp = _lib.LinkEstInputs(peer=dev_inputs[0], stats=dev_inputs[1], fwd=dev_inputs[2], K=int(dev_inputs[3]), reserved=0)
        check(self._L.rm_linkest_fold_device(self._h, C.byref(inp)))

    def linkest_read(self, nodes=None):
        """rm_linkest_read: (entries [n][K] of LINKEST_ENTRY_DTYPE, node state [n] of LINKEST_NODE_DTYPE -- the listed nodes in list
        order, or all --, the totals as a dict)"""
        ptr, n, _idx = self._node_list(nodes)
        K = max(self.linkest_enabled(), 1)
        ent = np.zeros((n, K), dtype=_lib.LINKEST_ENTRY_DTYPE)
        nod = np.zeros(n, dtype=_lib.LINKEST_NODE_DTYPE)
        tot = np.zeros(1, dtype=_lib.LINKEST_TOTALS_DTYPE)
        check(self._L.rm_linkest_read(self._h, ptr, n, ent.ctypes.data if n else None, nod.ctypes.data if n else None, tot.ctypes.data))
        return ent, nod, {k: int(tot[k][0]) for k in tot.dtype.names}

    def linkest_device(self):
        """rm_linkest_device: device pointers (entries [n_nodes][K] of 32 bytes, node state [n_nodes] of 32 bytes, totals)"""
        e, a, t = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self._L.rm_linkest_device(self._h, C.byref(e), C.byref(a), C.byref(t)))
        return e.value, a.value, t.value

    def linkest_tables(self):
        """rm_linkest_tables: the published table as etx_routes_device's dev_tables -- (peer pointer, stats pointer, K)"""
        t = _lib.EtxTables()
        check(self._L.rm_linkest_tables(self._h, C.byref(t)))
        return t.peer, t.stats, int(t.K)

    @staticmethod
    def linkest_fold_tables(peer, stats, fwd, params, entry, node, pub_peer, pub_stats, totals=None):
        """rm_linkest_fold_tables (pure host function): one fold over host arrays; entry (LINKEST_ENTRY_DTYPE [n][K]), node
        (LINKEST_NODE_DTYPE [n]), pub_peer (int32 [n][K]) and pub_stats (LINK_STATS_DTYPE [n][K]) change in place, totals
        (LINKEST_TOTALS_DTYPE [1], made when None) is added to -> totals"""
        keep = []
        inp = Engine._linkest_inputs(peer, stats, fwd, keep)
        n, K = keep[0].shape
        for a, dt, shape, what in ((entry, _lib.LINKEST_ENTRY_DTYPE, (n, K), "entry"), (node, _lib.LINKEST_NODE_DTYPE, (n,), "node"),
                                   (pub_peer, np.dtype(np.int32), (n, K), "pub_peer"), (pub_stats, _lib.LINK_STATS_DTYPE, (n, K), "pub_stats")):
            if a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError(what + " is a C-contiguous array of its record type, one row per node, updated in place")
        if totals is None:
            totals = np.zeros(1, dtype=_lib.LINKEST_TOTALS_DTYPE)
        check(_lib.lib().rm_linkest_fold_tables(n, C.byref(inp), C.byref(params), entry.ctypes.data, node.ctypes.data, pub_peer.ctypes.data,
                                                pub_stats.ctypes.data, totals.ctypes.data))
        return totals

    # -- java.util.Random
    def seed(self, seed):
        check(self._L.rm_seed(self._h, seed))

    @property
    def rng_state(self):
        s = C.c_uint64()
        check(self._L.rm_get_rng_state(self._h, C.byref(s)))
        return s.value

    @rng_state.setter
    def rng_state(self, v):
        check(self._L.rm_set_rng_state(self._h, v))

    # -- node state
    def upload_nodes(self, x, y, z=None, txpower=None, channel=None, enabled=None, rxprob=None, txprob=None,
                     int_id=None):
        def arr(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt)
        x = arr(x, np.float64)
        n = len(x)
        args = [x, arr(y, np.float64), arr(z, np.float64), arr(txpower, np.float64), arr(channel, np.int32),
                arr(enabled, np.uint8), arr(rxprob, np.float64), arr(txprob, np.float64), arr(int_id, np.int32)]
        for a in args:
            assert a is None or a.shape == (n,)
        check(self._L.rm_nodes_upload(self._h, n, *[_ptr(a) for a in args]))
        self.n = n

    def upload_table(self, nd):
        """nd: any object with x,y,z,txpower,channel,enabled,rxprob,txprob,int_id arrays."""
        self.upload_nodes(nd.x, nd.y, nd.z, nd.txpower, nd.channel, nd.enabled, nd.rxprob, nd.txprob, nd.int_id)

    def update_node(self, i, x, y, z, txpower, channel, enabled, rxprob, txprob):
        check(self._L.rm_node_update(self._h, i, x, y, z, txpower, channel, enabled, rxprob, txprob))

    def move_nodes(self, nodes, x, y, z=None):
        """New positions of several nodes in one call (rm_nodes_move)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        z = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
        check(self._L.rm_nodes_move(self._h, len(nodes), _ptr(nodes), _ptr(x), _ptr(y), _ptr(z)))

    def receiver_table_builds(self):
        return int(self._L.rm_receiver_table_builds(self._h))

    def set_partition(self, first, count):
        check(self._L.rm_set_partition(self._h, first, count))

    def set_partition_spatial(self, part, n_parts):
        """this context's receivers = region `part` of `n_parts` of the k-d split over all node positions"""
        check(self._L.rm_set_partition_spatial(self._h, part, n_parts))

    def partition_of_nodes(self, n_parts):
        """part owning every node under set_partition_spatial(., n_parts) (int32[n])"""
        out = np.empty(max(self.n, 1), dtype=np.int32)
        check(self._L.rm_partition_of_nodes(self._h, n_parts, out.ctypes.data))
        return out[: self.n]

    def partition_nodes(self):
        """node indices of this context's receivers, ascending"""
        out = np.empty(max(self.n, 1), dtype=np.int32)
        k = C.c_int32()
        check(self._L.rm_partition_nodes(self._h, out.ctypes.data, len(out), C.byref(k)))
        return out[: k.value].copy()

    def set_link_capacity(self, cap):
        check(self._L.rm_set_link_capacity(self._h, cap))

    def set_time(self, t):
        check(self._L.rm_set_time(self._h, t))

    def set_stream(self, stream_ptr):
        check(self._L.rm_set_stream(self._h, C.c_void_p(stream_ptr)))

    # -- transmit(): one packet
    def transmit(self, src, start_us=0, hex_length=0, txpower=None, channel=None, cap=None):
        cap = cap if cap is not None else max(1, self.n)
        dst = np.empty(cap, dtype=np.int32)
        verdict = np.empty(cap, dtype=np.uint8)
        rssi = np.empty(cap, dtype=np.float64)
        sinr = np.empty(cap, dtype=np.float64)
        cnt = C.c_uint32()
        interf = C.c_uint8()
        tp = C.byref(C.c_double(txpower)) if txpower is not None else None
        ch = C.byref(C.c_int32(channel)) if channel is not None else None
        check(self._L.rm_transmit(self._h, src, start_us, hex_length, tp, ch, dst.ctypes.data, verdict.ctypes.data,
                                  rssi.ctypes.data, sinr.ctypes.data, cap, C.byref(cnt), C.byref(interf)))
        k = cnt.value
        return TickResult(k, np.zeros(k, dtype=np.int32), dst[:k], verdict[:k], rssi[:k], sinr[:k],
                          np.array([interf.value], dtype=np.uint8), np.array([0, k], dtype=np.uint32))

    # -- batched tick (host records)
    def tick_begin(self, t_begin, t_end):
        check(self._L.rm_tick_begin(self._h, t_begin, t_end))
        self._n_new = 0

    def enqueue_tx(self, src, start_us, air_us, txpower=None, channel=None):
        tp = C.byref(C.c_double(txpower)) if txpower is not None else None
        ch = C.byref(C.c_int32(channel)) if channel is not None else None
        check(self._L.rm_enqueue_tx(self._h, src, start_us, air_us, tp, ch))
        self._n_new += 1

    def enqueue_records(self, recs):
        recs = np.ascontiguousarray(recs, dtype=TX_RECORD_DTYPE)
        check(self._L.rm_enqueue_tx_records(self._h, recs.ctypes.data, len(recs)))
        self._n_new += len(recs)

    def tick_flush(self, cap=None):
        n_new = self._n_new
        cap = cap if cap is not None else max(1, n_new) * max(1, self.n)
        cap = min(cap, 1 << 26)
        pkt = np.empty(cap, dtype=np.int32)
        dst = np.empty(cap, dtype=np.int32)
        verdict = np.empty(cap, dtype=np.uint8)
        rssi = np.empty(cap, dtype=np.float64)
        sinr = np.empty(cap, dtype=np.float64)
        pint = np.zeros(max(1, n_new), dtype=np.uint8)
        poff = np.zeros(n_new + 1, dtype=np.uint32)
        cnt = C.c_uint32()
        check(self._L.rm_tick_flush(self._h, pkt.ctypes.data, dst.ctypes.data, verdict.ctypes.data, rssi.ctypes.data,
                                    sinr.ctypes.data, cap, C.byref(cnt), pint.ctypes.data, poff.ctypes.data))
        k = cnt.value
        return TickResult(k, pkt[:k], dst[:k], verdict[:k], rssi[:k], sinr[:k], pint[:n_new], poff)

    @staticmethod
    def _wrap_host_result(r):
        return HostTickView(r)

    def batch_result_view(self, n_slots, raise_on_error=True):
        """Results of slots 0..n_slots-1 of the last batch, wrapped in place in the engine's pinned host
        block (one packing launch, one wait).  Returns (results, status per slot)."""
        res = (HostResult * n_slots)()
        status = (C.c_int32 * n_slots)()
        rc = self._L.rm_batch_result_view(self._h, n_slots, res, status)
        if rc != 0 and (raise_on_error or all(s == 0 for s in status)):
            check(rc)
        return [self._wrap_host_result(r) for r in res], list(status)

    def tick_flush_view(self):
        """Evaluate the enqueued tick; the result stays in the engine's pinned host block and is wrapped,
        not copied (valid until the next evaluating call on this engine)."""
        n_new = self._n_new
        r = HostResult()
        check(self._L.rm_tick_flush_view(self._h, C.byref(r)))
        assert r.n_packets == n_new
        return self._wrap_host_result(r)

    def tick_run(self):
        """Evaluate the enqueued tick; results stay on the device (result_copy / result_device)."""
        check(self._L.rm_tick_run(self._h))

    def draws_pending(self):
        return bool(self._L.rm_draws_pending(self._h))

    def draw_counts_device(self):
        p, n = C.c_void_p(), C.c_int32()
        check(self._L.rm_draw_counts_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def draw_counts_to(self, dev_out_ptr):
        check(self._L.rm_draw_counts_to(self._h, C.c_void_p(dev_out_ptr)))

    def finish_draws(self, all_counts, world, rank):
        """all_counts: host uint32 array [world, n_new] or a device pointer (int)."""
        if isinstance(all_counts, int):
            check(self._L.rm_tick_finish_draws(self._h, C.c_void_p(all_counts), world, rank, 1))
        else:
            a = np.ascontiguousarray(all_counts, dtype=np.uint32)
            check(self._L.rm_tick_finish_draws(self._h, a.ctypes.data, world, rank, 0))

    def draw_nodes_device(self):
        """device pointer of the node index of every link of the last tick that will draw (spatial partitions)"""
        p = C.c_void_p()
        check(self._L.rm_draw_nodes_device(self._h, C.byref(p)))
        return p.value

    def finish_draws_nodes(self, all_counts, all_nodes, stride, world):
        """spatial partitions: all_counts [world, n_new] uint32 and all_nodes [world, stride] int32, host arrays or device
        pointers (both ints)"""
        if isinstance(all_counts, int):
            check(self._L.rm_tick_finish_draws_nodes(self._h, C.c_void_p(all_counts), C.c_void_p(all_nodes), stride, world, 1))
        else:
            a = np.ascontiguousarray(all_counts, dtype=np.uint32)
            b = np.ascontiguousarray(all_nodes, dtype=np.int32)
            check(self._L.rm_tick_finish_draws_nodes(self._h, a.ctypes.data, b.ctypes.data, stride, world, 0))

    def tick(self, recs, t_begin=0, t_end=0, cap=None):
        self.tick_begin(t_begin, t_end)
        self.enqueue_records(recs)
        return self.tick_flush(cap)

    # -- device-resident path
    def pack_tx_device(self, dev_src_ptr, n, start_us, air_us, dev_out_ptr):
        check(self._L.rm_pack_tx_device(self._h, C.c_void_p(dev_src_ptr), n, start_us, air_us,
                                        C.c_void_p(dev_out_ptr)))

    def pack_tx_device_on(self, stream_ptr, dev_src_ptr, n, start_us, air_us, dev_out_ptr):
        check(self._L.rm_pack_tx_device_on(self._h, C.c_void_p(stream_ptr), C.c_void_p(dev_src_ptr), n, start_us, air_us,
                                           C.c_void_p(dev_out_ptr)))

    def pack_tx_batch_device_on(self, stream_ptr, dev_src_ptr, n_ticks, n, start_us, air_us, dev_out_ptr):
        st = np.ascontiguousarray(start_us, dtype=np.int64)
        assert len(st) == n_ticks
        check(self._L.rm_pack_tx_batch_device_on(self._h, C.c_void_p(stream_ptr), C.c_void_p(dev_src_ptr), n_ticks, n,
                                                 st.ctypes.data, air_us, C.c_void_p(dev_out_ptr)))

    def tick_run_device(self, t_begin, t_end, dev_new_ptr, n_new):
        check(self._L.rm_tick_run_device(self._h, t_begin, t_end, C.c_void_p(dev_new_ptr), n_new))

    def tick_run_records_device(self, t_begin, t_end, dev_new_ptr, n_new, latest_end_us):
        """records in device memory for the SINR medium, whose frames stay on the air: `latest_end_us` bounds start + air"""
        check(self._L.rm_tick_run_records_device(self._h, int(t_begin), int(t_end), C.c_void_p(dev_new_ptr), int(n_new), int(latest_end_us)))

    def tick_run_sources_device(self, t_begin, t_end, dev_src_ptr, n, start_us, air_us):
        check(self._L.rm_tick_run_sources_device(self._h, t_begin, t_end, C.c_void_p(dev_src_ptr), n, start_us, air_us))

    # -- several independent ticks per pass (rm_batch_*)
    def batch_run_sources_device(self, t_begin, t_end, dev_src_ptrs, n_src, start_us, air_us):
        """Tick b: sources dev_src_ptrs[b] (device int32[n_src[b]]), frames start at start_us[b]."""
        n = len(dev_src_ptrs)
        i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
        tb, te, st, ai = i64(t_begin), i64(t_end), i64(start_us), i64(air_us)
        ptrs = np.ascontiguousarray(dev_src_ptrs, dtype=np.uint64)
        cnt = np.ascontiguousarray(n_src, dtype=np.int32)
        assert len(tb) == len(te) == len(st) == len(ai) == len(cnt) == n
        check(self._L.rm_batch_run_sources_device(self._h, n, tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data,
                                                  cnt.ctypes.data, st.ctypes.data, ai.ctypes.data))

    def batch_run_device(self, t_begin, t_end, dev_rec_ptrs, n_new):
        n = len(dev_rec_ptrs)
        tb = np.ascontiguousarray(t_begin, dtype=np.int64)
        te = np.ascontiguousarray(t_end, dtype=np.int64)
        ptrs = np.ascontiguousarray(dev_rec_ptrs, dtype=np.uint64)
        cnt = np.ascontiguousarray(n_new, dtype=np.int32)
        assert len(tb) == len(te) == len(cnt) == n
        check(self._L.rm_batch_run_device(self._h, n, tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data, cnt.ctypes.data))

    def batch_run_gathered_device(self, t_begin, t_end, dev_gathered_ptr, world, slots):
        """the ticks' records where an all-gather of per-rank blocks left them: [rank][tick][slot]"""
        tb = np.ascontiguousarray(t_begin, dtype=np.int64)
        te = np.ascontiguousarray(t_end, dtype=np.int64)
        check(self._L.rm_batch_run_gathered_device(self._h, len(tb), tb.ctypes.data, te.ctypes.data, C.c_void_p(dev_gathered_ptr),
                                                   world, slots))

    def batch_run_gathered_sources_device(self, t_begin, t_end, dev_src_all_ptr, world, slots, start_us, air_us):
        """the ticks' source indices where an all-gather of per-rank blocks left them: [rank][tick][slot] (-1: padding)"""
        tb = np.ascontiguousarray(t_begin, dtype=np.int64)
        te = np.ascontiguousarray(t_end, dtype=np.int64)
        st = np.ascontiguousarray(start_us, dtype=np.int64)
        check(self._L.rm_batch_run_gathered_sources_device(self._h, len(tb), tb.ctypes.data, te.ctypes.data, C.c_void_p(dev_src_all_ptr),
                                                           world, slots, st.ctypes.data, int(air_us)))

    GATHER_TRAILER = 4   # RM_GATHER_TRAILER: words behind a rank's source indices in its block (digest low, high, two spare)

    def batch_tile_reuse(self):
        """ticks of the last batch a filter workgroup swept with one load of its receivers"""
        return int(self._L.rm_batch_tile_reuse(self._h))

    def table_digest(self):
        """rm_table_digest: a function of the node table's content as this context holds it"""
        d = C.c_uint64(0)
        check(self._L.rm_table_digest(self._h, C.byref(d)))
        return int(d.value)

    @staticmethod
    def gather_blocks(per_rank_sources, digests):
        """what the library's all-gather of a sharded batch delivers: per rank its [ticks][slots] source indices, then the
        trailer with the rank's table digest -> int32 [world][ticks * slots + GATHER_TRAILER]"""
        rows = []
        for src, dg in zip(per_rank_sources, digests):
            flat = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
            tr = np.array([dg & 0xFFFFFFFF, (dg >> 32) & 0xFFFFFFFF, 0, 0], dtype=np.uint32).view(np.int32)
            rows.append(np.concatenate([flat, tr]))
        return np.stack(rows)

    def batch_run_gathered_blocks_device(self, t_begin, t_end, dev_blocks_ptr, world, slots, start_us, air_us):
        """as batch_run_gathered_sources_device with every rank's block followed by its trailer (gather_blocks): the ranks'
        node-table digests are compared with this context's on the device"""
        tb = np.ascontiguousarray(t_begin, dtype=np.int64)
        te = np.ascontiguousarray(t_end, dtype=np.int64)
        st = np.ascontiguousarray(start_us, dtype=np.int64)
        check(self._L.rm_batch_run_gathered_blocks_device(self._h, len(tb), tb.ctypes.data, te.ctypes.data, C.c_void_p(dev_blocks_ptr),
                                                          world, slots, st.ctypes.data, int(air_us)))

    def prepared(self, name, *args):
        """A call with its arguments converted once: `name` is an entry point that takes the context first; numpy arrays are
        passed by address (and kept alive by the closure).  The returned function costs one ctypes call -- what a host
        loop that issues the same shape of call thousands of times wants (bench.py's timed region)."""
        fn = getattr(self._L, name)
        keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
        conv = [C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in keep]
        h = self._h

        def call(_fn=fn, _h=h, _conv=tuple(conv), _keep=keep):
            rc = _fn(_h, *_conv)
            if rc != 0:
                check(rc)
        return call

    # -- RCCL inside the library (rm_comm_*, rm_dist_*)
    @staticmethod
    def comm_available():
        return bool(_lib.lib().rm_comm_available())

    @staticmethod
    def comm_unique_id():
        buf = np.zeros(128, dtype=np.uint8)
        check(_lib.lib().rm_comm_get_unique_id(buf.ctypes.data))
        return buf

    def comm_init_rank(self, unique_id, world, rank):
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        check(self._L.rm_comm_init_rank(self._h, uid.ctypes.data, world, rank))

    def comm_destroy(self):
        check(self._L.rm_comm_destroy(self._h))

    def dist_batch_run_sources_device(self, t_begin, t_end, dev_src_ptr, slots, start_us, air_us):
        """one batch of a receiver-sharded run: pack this rank's transmitters (rows of `slots` node indices), RCCL
        all-gather, sweep -- one call"""
        tb = np.ascontiguousarray(t_begin, dtype=np.int64)
        te = np.ascontiguousarray(t_end, dtype=np.int64)
        st = np.ascontiguousarray(start_us, dtype=np.int64)
        check(self._L.rm_dist_batch_run_sources_device(self._h, len(tb), tb.ctypes.data, te.ctypes.data, C.c_void_p(dev_src_ptr),
                                                       slots, st.ctypes.data, int(air_us)))

    def dist_tick_run_sources_device(self, t_begin, t_end, dev_src_ptr, slots, start_us, air_us):
        check(self._L.rm_dist_tick_run_sources_device(self._h, int(t_begin), int(t_end), C.c_void_p(dev_src_ptr), slots,
                                                      int(start_us), int(air_us)))

    def batch_result_device(self, slot):
        r = DeviceResult()
        check(self._L.rm_batch_result_device(self._h, slot, C.byref(r)))
        return r

    def batch_result_count(self, slot):
        cnt, dropped = C.c_uint32(), C.c_uint32()
        check(self._L.rm_batch_result_count(self._h, slot, C.byref(cnt), C.byref(dropped)))
        return cnt.value, dropped.value

    def batch_result_copy(self, slot, n_new, cap=None):
        """Heard links of tick `slot` of the last batch, copied to the host."""
        cap = cap if cap is not None else min(max(1, n_new) * max(1, self.n), 1 << 26)
        pkt = np.empty(cap, dtype=np.int32)
        dst = np.empty(cap, dtype=np.int32)
        verdict = np.empty(cap, dtype=np.uint8)
        rssi = np.empty(cap, dtype=np.float64)
        sinr = np.empty(cap, dtype=np.float64)
        pint = np.zeros(max(1, n_new), dtype=np.uint8)
        poff = np.zeros(n_new + 1, dtype=np.uint32)
        cnt = C.c_uint32()
        check(self._L.rm_batch_result_copy(self._h, slot, pkt.ctypes.data, dst.ctypes.data, verdict.ctypes.data,
                                           rssi.ctypes.data, sinr.ctypes.data, cap, C.byref(cnt), pint.ctypes.data,
                                           poff.ctypes.data))
        k = cnt.value
        return TickResult(k, pkt[:k], dst[:k], verdict[:k], rssi[:k], sinr[:k], pint[:n_new], poff)

    def result_dense(self):
        """rm_result_dense: the dense tick's heard links as lane masks per (packet, 1024 nodes) cell -- device pointers"""
        r = _lib.DenseResult()
        check(self._L.rm_result_dense(self._h, C.byref(r)))
        return r

    def result_device(self):
        r = DeviceResult()
        check(self._L.rm_result_device(self._h, C.byref(r)))
        return r

    def result_copy(self, n_new, cap=None):
        """Heard links of the last device-path tick, copied to the host."""
        cap = cap if cap is not None else min(max(1, n_new) * max(1, self.n), 1 << 26)
        pkt = np.empty(cap, dtype=np.int32)
        dst = np.empty(cap, dtype=np.int32)
        verdict = np.empty(cap, dtype=np.uint8)
        rssi = np.empty(cap, dtype=np.float64)
        sinr = np.empty(cap, dtype=np.float64)
        pint = np.zeros(max(1, n_new), dtype=np.uint8)
        poff = np.zeros(n_new + 1, dtype=np.uint32)
        cnt = C.c_uint32()
        check(self._L.rm_result_copy(self._h, pkt.ctypes.data, dst.ctypes.data, verdict.ctypes.data, rssi.ctypes.data,
                                     sinr.ctypes.data, cap, C.byref(cnt), pint.ctypes.data, poff.ctypes.data))
        k = cnt.value
        return TickResult(k, pkt[:k], dst[:k], verdict[:k], rssi[:k], sinr[:k], pint[:n_new], poff)

    def result_count(self):
        cnt, dropped = C.c_uint32(), C.c_uint32()
        check(self._L.rm_result_count(self._h, C.byref(cnt), C.byref(dropped)))
        return cnt.value, dropped.value

    # ---- reception stage (Simulator.generate*Events + processAllEvents + Transciever state on the device)
    def events_enable(self, max_packets=0, max_links=0):
        check(self._L.rm_events_enable(self._h, max_packets, max_links))

    def events_disable(self):
        check(self._L.rm_events_disable(self._h))

    def events_next_packet(self):
        return self._L.rm_events_next_packet(self._h)

    def events_process(self, time_us, copy=True, runs=False):
        """Simulator.emulatorTimeStepDone: currentTime = time; processAllEvents(time).  Returns the deliveries of
        the drain in call order: (packet numbers, destination node indices, rssi, pending packets), copied out of the pinned
        block (copy=False: wrapped in place, valid until the next call).  runs=True: as the engine hands them over -- the
        packet numbers once per run of deliveries: (run packet, run first, run count, destinations, rssi, pending packets)."""
        from ._lib import DeliveryView
        v = DeliveryView()
        check(self._L.rm_events_process(self._h, int(time_us), C.byref(v)))
        self.oldest_pending_packet = v.oldest_packet   # every packet below it has fired its last event
        return self._delivery_tuple(v, copy, runs)

    def events_process_batch(self, times, copy=True, runs=False):
        """The ticks of the last batch_run_device / batch_run_sources_device handed to the reception stage, slot b as tick b, each
        followed by the drain events_process(times[b]) -- the same deliveries, bit for bit, as lone ticks and drains in turn.
        Returns one tuple per tick, shaped as events_process returns it (copy=False: wrapped in place, valid until the next
        events_process* call)."""
        from ._lib import DeliveryView
        t = np.ascontiguousarray(times, dtype=np.int64)
        n = len(t)
        views = (DeliveryView * max(n, 1))()
        check(self._L.rm_events_process_batch(self._h, n, t.ctypes.data, views))
        self.oldest_pending_packets = [views[b].oldest_packet for b in range(n)]   # per tick, as events_process leaves it
        if n:
            self.oldest_pending_packet = views[n - 1].oldest_packet
        return [self._delivery_tuple(views[b], copy, runs) for b in range(n)]

    @staticmethod
    def _delivery_tuple(v, copy, runs):
        k = v.count

        def arr(ptr, dtype, count=k):
            a = _wrap(ptr, dtype, count)
            return a.copy() if copy else a
        # the packet numbers come once per run of deliveries (a packet's deliveries are adjacent): spread out here
        n_runs = v.n_runs
        if runs:
            return (arr(v.run_packet, np.int64, n_runs), arr(v.run_first, np.uint32, n_runs), arr(v.run_count, np.uint32, n_runs),
                    arr(v.dst, np.int32), arr(v.rssi, np.float64), v.pending_packets)
        first, cnt = _wrap(v.run_first, np.uint32, n_runs), _wrap(v.run_count, np.uint32, n_runs)
        assert n_runs == 0 or (first[0] == 0 and int(first[-1]) + int(cnt[-1]) == k and np.all(first[1:] == (first[:-1] + cnt[:-1])))
        packet = np.repeat(_wrap(v.run_packet, np.int64, n_runs), cnt)
        return packet, arr(v.dst, np.int32), arr(v.rssi, np.float64), v.pending_packets

    def node_info(self, nodes=None, n=None):
        """(rssi, receiving state, channel) per node: the node-info of a time-step message."""
        if nodes is not None:
            nodes = np.ascontiguousarray(nodes, dtype=np.int32)
            n = len(nodes)
        elif n is None:
            n = self._L.rm_node_count(self._h)
        rssi = np.empty(n, dtype=np.float64)
        rx = np.empty(n, dtype=np.int32)
        ch = np.empty(n, dtype=np.int32)
        check(self._L.rm_node_info(self._h, nodes.ctypes.data if nodes is not None else None, n, rssi.ctypes.data,
                                   rx.ctypes.data, ch.ctypes.data))
        return rssi, rx, ch

    def node_info_changed(self):
        """(nodes, rssi, receiving, channel) of the nodes whose node-info differs from what this call reported for them last"""
        n = max(self.n, 1)
        nodes = np.empty(n, dtype=np.int32)
        rssi = np.empty(n, dtype=np.float64)
        rx = np.empty(n, dtype=np.int32)
        ch = np.empty(n, dtype=np.int32)
        k = C.c_int32(0)
        check(self._L.rm_node_info_changed(self._h, nodes.ctypes.data, rssi.ctypes.data, rx.ctypes.data, ch.ctypes.data, n, C.byref(k)))
        return nodes[:k.value], rssi[:k.value], rx[:k.value], ch[:k.value]

    def channel_energy(self, time_us, nodes=None, channel=None, cca_threshold_dbm=float("nan")):
        """(energy in dBm, flags) per node -- all nodes, or the listed ones -- at `time_us`, over the frames on the air of the SINR
        medium; channel None: every node on its own channel.  flags: ED_TRANSMITTING | ED_BUSY."""
        if nodes is not None:
            nodes = np.ascontiguousarray(nodes, dtype=np.int32)
            n = len(nodes)
        else:
            n = self._L.rm_node_count(self._h)
        energy = np.empty(n, dtype=np.float64)
        flags = np.empty(n, dtype=np.uint8)
        check(self._L.rm_channel_energy(self._h, int(time_us), nodes.ctypes.data if nodes is not None else None, n,
                                        _lib.CHANNEL_OWN if channel is None else int(channel), float(cca_threshold_dbm),
                                        energy.ctypes.data, flags.ctypes.data))
        return energy, flags

    def channel_energy_device(self, time_us, dev_nodes_ptr, n, channel, cca_threshold_dbm, dev_energy_ptr, dev_flags_ptr):
        """The raw form: device pointers, asynchronous on the context's stream (dev_nodes_ptr None: nodes 0 .. n-1)."""
        check(self._L.rm_channel_energy_device(self._h, int(time_us), dev_nodes_ptr, int(n),
                                               _lib.CHANNEL_OWN if channel is None else int(channel), float(cca_threshold_dbm),
                                               dev_energy_ptr, dev_flags_ptr))

    def tick_run_sources_cca(self, t_begin, t_end, src, start_us, air_us, cca_time_us, cca_threshold_dbm=float("nan")):
        """A carrier-sense gated tick: the candidates `src` (node indices, -1 = padding) are sensed at
        `cca_time_us` on the device and only the ones with flags 0 go on the air.  -> (flags, energy in dBm) per candidate; the
        tick's results through result_copy(len(src)) as after tick_run_sources_device."""
        src = np.ascontiguousarray(src, dtype=np.int32)
        n = len(src)
        flags = np.empty(n, dtype=np.uint8)
        energy = np.empty(n, dtype=np.float64)
        check(self._L.rm_tick_run_sources_cca(self._h, int(t_begin), int(t_end), src.ctypes.data, n, int(start_us), int(air_us),
                                              int(cca_time_us), float(cca_threshold_dbm), flags.ctypes.data, energy.ctypes.data))
        return flags, energy

    def tick_run_sources_cca_device(self, t_begin, t_end, dev_src_ptr, n, start_us, air_us, cca_time_us, cca_threshold_dbm,
                                    dev_flags_ptr=None, dev_energy_ptr=None):
        """The raw form: device pointers, asynchronous on the context's stream; the caller's list is not written."""
        check(self._L.rm_tick_run_sources_cca_device(self._h, int(t_begin), int(t_end), dev_src_ptr, int(n), int(start_us), int(air_us),
                                                     int(cca_time_us), float(cca_threshold_dbm), dev_flags_ptr, dev_energy_ptr))

    def _cca_batch_args(self, t_begin, t_end, n_src, start_us, air_us, cca_time_us):
        i64 = lambda v: np.ascontiguousarray(v, dtype=np.int64)
        tb, te, st, ai, tc = i64(t_begin), i64(t_end), i64(start_us), i64(air_us), i64(cca_time_us)
        cnt = np.ascontiguousarray(n_src, dtype=np.int32)
        assert len(tb) == len(te) == len(st) == len(ai) == len(tc) == len(cnt)
        return tb, te, st, ai, tc, cnt

    def batch_run_sources_cca(self, t_begin, t_end, src_lists, start_us, air_us, cca_time_us, cca_threshold_dbm=float("nan")):
        """A carrier-sense gated batch: tick b's candidates src_lists[b] (node indices, -1 = padding) are
        sensed at cca_time_us[b] over the window plus the kept frames of the earlier ticks of the batch.  -> (flags, energy in dBm),
        one array per tick; the ticks' results through batch_result_copy(b, len(src_lists[b])) as after batch_run_sources_device."""
        lists = [np.ascontiguousarray(s, dtype=np.int32) for s in src_lists]
        tb, te, st, ai, tc, cnt = self._cca_batch_args(t_begin, t_end, [len(s) for s in lists], start_us, air_us, cca_time_us)
        assert len(lists) == len(tb)
        ptrs = np.array([s.ctypes.data if len(s) else 0 for s in lists], dtype=np.uint64)
        total = int(cnt.sum())
        flags = np.empty(max(total, 1), dtype=np.uint8)
        energy = np.empty(max(total, 1), dtype=np.float64)
        check(self._L.rm_batch_run_sources_cca(self._h, len(lists), tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data, cnt.ctypes.data,
                                               st.ctypes.data, ai.ctypes.data, tc.ctypes.data, float(cca_threshold_dbm),
                                               flags.ctypes.data, energy.ctypes.data))
        cuts = np.cumsum(cnt)[:-1]
        return np.split(flags[:total], cuts), np.split(energy[:total], cuts)

    def batch_run_sources_cca_device(self, t_begin, t_end, dev_src_ptrs, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm,
                                     dev_flags_ptr=None, dev_energy_ptr=None):
        """The raw form: device lists, flat device outputs in tick order (sum(n_src) entries each, or None); the callers' lists are
        not written."""
        tb, te, st, ai, tc, cnt = self._cca_batch_args(t_begin, t_end, n_src, start_us, air_us, cca_time_us)
        ptrs = np.ascontiguousarray([p or 0 for p in dev_src_ptrs], dtype=np.uint64)
        assert len(ptrs) == len(tb)
        check(self._L.rm_batch_run_sources_cca_device(self._h, len(ptrs), tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data, cnt.ctypes.data,
                                                      st.ctypes.data, ai.ctypes.data, tc.ctypes.data, float(cca_threshold_dbm),
                                                      dev_flags_ptr, dev_energy_ptr))

    @staticmethod
    def csma_params(max_backoffs=None, min_be=None, max_be=None, seed=None, reserved=None):
        """rm_csma_params: the library's defaults (4, 3, 5, seed 0) with the given fields replaced"""
        p = _lib.CsmaParams()
        _lib.lib().rm_csma_defaults(C.byref(p))
        for name, v in (("max_backoffs", max_backoffs), ("min_be", min_be), ("max_be", max_be), ("seed", seed), ("reserved", reserved)):
            if v is not None:
                setattr(p, name, int(v))
        return p

    @staticmethod
    def csma_schedule(params, n_src, cca_time_us, cap=None):
        """The CSMA-CA schedule of a batch, on the host alone: -> (n_exp per tick, origin per expanded slot --
        a flat packet index --, attempt per expanded slot); cap: the room offered for origin / attempt (default: what is needed)."""
        cnt = np.ascontiguousarray(n_src, dtype=np.int32)
        tc = np.ascontiguousarray(cca_time_us, dtype=np.int64)
        assert len(cnt) == len(tc)
        n_exp = np.zeros(len(cnt), dtype=np.int32)
        total = C.c_int64(-1)
        L = _lib.lib()
        if cap is None:
            check(L.rm_csma_schedule(C.byref(params), len(cnt), cnt.ctypes.data, tc.ctypes.data, n_exp.ctypes.data, None, None, 0, C.byref(total)))
            cap = total.value
        origin = np.zeros(max(int(cap), 1), dtype=np.int32)
        attempt = np.zeros(max(int(cap), 1), dtype=np.uint8)
        try:
            check(L.rm_csma_schedule(C.byref(params), len(cnt), cnt.ctypes.data, tc.ctypes.data, n_exp.ctypes.data, origin.ctypes.data,
                                     attempt.ctypes.data, int(cap), C.byref(total)))
        except _lib.RadioMediumError as err:
            err.total = total.value
            raise
        return n_exp, origin[:total.value], attempt[:total.value]

    CSMA_FIELDS = (("status", np.uint8), ("attempts", np.uint8), ("tick", np.int32), ("pkt", np.int32), ("flags", np.uint8),
                   ("energy_dbm", np.float64))

    def batch_run_sources_csma(self, t_begin, t_end, src_lists, start_us, air_us, cca_time_us, cca_threshold_dbm, params, fields=None):
        """A CSMA-CA gated batch: the gated batch in which a deferred candidate backs off and senses again in a
        later tick.  -> ({field: flat array over the packets}, n_exp per tick); the ticks' results through batch_result_copy(b, n_exp[b]).
        fields: the outputs to ask for (default: all of CSMA_FIELDS)."""
        lists = [np.ascontiguousarray(s, dtype=np.int32) for s in src_lists]
        tb, te, st, ai, tc, cnt = self._cca_batch_args(t_begin, t_end, [len(s) for s in lists], start_us, air_us, cca_time_us)
        assert len(lists) == len(tb)
        ptrs = np.array([s.ctypes.data if len(s) else 0 for s in lists], dtype=np.uint64)
        total = int(cnt.sum())
        want = [f for f, _ in self.CSMA_FIELDS] if fields is None else list(fields)
        out = {f: np.empty(max(total, 1), dtype=t) for f, t in self.CSMA_FIELDS if f in want}
        res = _lib.CsmaResult(**{f: a.ctypes.data for f, a in out.items()})
        n_exp = np.zeros(len(lists), dtype=np.int32)
        check(self._L.rm_batch_run_sources_csma(self._h, len(lists), tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data, cnt.ctypes.data,
                                                st.ctypes.data, ai.ctypes.data, tc.ctypes.data, float(cca_threshold_dbm), C.byref(params),
                                                C.byref(res), n_exp.ctypes.data))
        return {f: a[:total] for f, a in out.items()}, n_exp

    def batch_run_sources_csma_device(self, t_begin, t_end, dev_src_ptrs, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, params,
                                      dev_out=None):
        """The raw form: device lists; dev_out: {field: device pointer} for the outputs wanted (flat, sum(n_src) entries each); the
        callers' lists are not written.  -> n_exp per tick."""
        tb, te, st, ai, tc, cnt = self._cca_batch_args(t_begin, t_end, n_src, start_us, air_us, cca_time_us)
        ptrs = np.ascontiguousarray([p or 0 for p in dev_src_ptrs], dtype=np.uint64)
        assert len(ptrs) == len(tb)
        res = _lib.CsmaResult(**(dev_out or {}))
        n_exp = np.zeros(len(ptrs), dtype=np.int32)
        check(self._L.rm_batch_run_sources_csma_device(self._h, len(ptrs), tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data, cnt.ctypes.data,
                                                       st.ctypes.data, ai.ctypes.data, tc.ctypes.data, float(cca_threshold_dbm),
                                                       C.byref(params), C.byref(res) if dev_out is not None else None, n_exp.ctypes.data))
        return n_exp

    # ---- the carry of a CSMA-CA gated batch: pending packets go on in the next batch
    CSMA_CARRY_DTYPE = np.dtype([("origin_cca_time_us", "<i8"), ("origin_slot", "<i4"), ("node", "<i4"), ("tick", "<i4"), ("attempt", "<i4")])

    @classmethod
    def _carry(cls, carry):
        """rm_csma_carry[]: a structured array of CSMA_CARRY_DTYPE (None: an empty list) -> (contiguous array, pointer or None)"""
        a = np.zeros(0, dtype=cls.CSMA_CARRY_DTYPE) if carry is None else np.ascontiguousarray(carry, dtype=cls.CSMA_CARRY_DTYPE)
        assert a.ndim == 1 and a.dtype.itemsize == C.sizeof(_lib.CsmaCarry)
        return a, (a.ctypes.data if len(a) else None)

    @classmethod
    def csma_schedule_carry(cls, params, n_src, cca_time_us, carry, cap=None):
        """csma_schedule with a carry list (E9): in origin a carried slot is sum(n_src) + its place in the carry list"""
        cnt = np.ascontiguousarray(n_src, dtype=np.int32)
        tc = np.ascontiguousarray(cca_time_us, dtype=np.int64)
        assert len(cnt) == len(tc)
        car, car_p = cls._carry(carry)
        n_exp = np.zeros(len(cnt), dtype=np.int32)
        total = C.c_int64(-1)
        L = _lib.lib()
        if cap is None:
            check(L.rm_csma_schedule_carry(C.byref(params), len(cnt), cnt.ctypes.data, tc.ctypes.data, car_p, len(car), n_exp.ctypes.data, None,
                                           None, 0, C.byref(total)))
            cap = total.value
        origin = np.zeros(max(int(cap), 1), dtype=np.int32)
        attempt = np.zeros(max(int(cap), 1), dtype=np.uint8)
        try:
            check(L.rm_csma_schedule_carry(C.byref(params), len(cnt), cnt.ctypes.data, tc.ctypes.data, car_p, len(car), n_exp.ctypes.data,
                                           origin.ctypes.data, attempt.ctypes.data, int(cap), C.byref(total)))
        except _lib.RadioMediumError as err:
            err.total = total.value
            raise
        return n_exp, origin[:total.value], attempt[:total.value]

    def batch_run_sources_csma_carry(self, t_begin, t_end, src_lists, start_us, air_us, cca_time_us, cca_threshold_dbm, params, carry,
                                     fields=None, carried_fields=None):
        """batch_run_sources_csma with carried packets (E9; carry: a structured array of CSMA_CARRY_DTYPE or None).
        -> ({field: per own packet}, {field: per carried packet}, n_exp per tick)"""
        lists = [np.ascontiguousarray(s, dtype=np.int32) for s in src_lists]
        tb, te, st, ai, tc, cnt = self._cca_batch_args(t_begin, t_end, [len(s) for s in lists], start_us, air_us, cca_time_us)
        assert len(lists) == len(tb)
        ptrs = np.array([s.ctypes.data if len(s) else 0 for s in lists], dtype=np.uint64)
        car, car_p = self._carry(carry)
        total = int(cnt.sum())
        tables = []
        for n, names in ((total, fields), (len(car), carried_fields)):
            want = [f for f, _ in self.CSMA_FIELDS] if names is None else list(names)
            tables.append({f: np.empty(max(n, 1), dtype=t) for f, t in self.CSMA_FIELDS if f in want})
        res = [_lib.CsmaResult(**{f: a.ctypes.data for f, a in t.items()}) for t in tables]
        n_exp = np.zeros(len(lists), dtype=np.int32)
        check(self._L.rm_batch_run_sources_csma_carry(self._h, len(lists), tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data, cnt.ctypes.data,
                                                      st.ctypes.data, ai.ctypes.data, tc.ctypes.data, float(cca_threshold_dbm), C.byref(params),
                                                      C.byref(res[0]), n_exp.ctypes.data, car_p, len(car), C.byref(res[1])))
        return {f: a[:total] for f, a in tables[0].items()}, {f: a[:len(car)] for f, a in tables[1].items()}, n_exp

    def batch_run_sources_csma_carry_device(self, t_begin, t_end, dev_src_ptrs, n_src, start_us, air_us, cca_time_us, cca_threshold_dbm, params,
                                            carry, dev_out=None, dev_carried_out=None):
        """The raw form: device lists; dev_out / dev_carried_out: {field: device pointer} (sum(n_src) / len(carry) entries each); the
        carry list itself is a host array.  -> n_exp per tick."""
        tb, te, st, ai, tc, cnt = self._cca_batch_args(t_begin, t_end, n_src, start_us, air_us, cca_time_us)
        ptrs = np.ascontiguousarray([p or 0 for p in dev_src_ptrs], dtype=np.uint64)
        assert len(ptrs) == len(tb)
        car, car_p = self._carry(carry)
        res, res_c = _lib.CsmaResult(**(dev_out or {})), _lib.CsmaResult(**(dev_carried_out or {}))
        n_exp = np.zeros(len(ptrs), dtype=np.int32)
        check(self._L.rm_batch_run_sources_csma_carry_device(self._h, len(ptrs), tb.ctypes.data, te.ctypes.data, ptrs.ctypes.data,
                                                             cnt.ctypes.data, st.ctypes.data, ai.ctypes.data, tc.ctypes.data,
                                                             float(cca_threshold_dbm), C.byref(params),
                                                             C.byref(res) if dev_out is not None else None, n_exp.ctypes.data, car_p, len(car),
                                                             C.byref(res_c) if dev_carried_out is not None else None))
        return n_exp

    @classmethod
    def csma_carry_collect(cls, src_lists, cca_time_us, carry, out, carried_out, cap=None):
        """The next batch's carry list from a batch's host results (E9; no device needed): the pending carried packets in carry-in order,
        then the pending own packets in flat order.  out / carried_out: {field: array} with status, attempts and tick.
        cap: the room offered (default: every packet); too small: RadioMediumError with .count."""
        lists = [np.ascontiguousarray(s, dtype=np.int32) for s in src_lists]
        cnt = np.array([len(s) for s in lists], dtype=np.int32)
        tc = np.ascontiguousarray(cca_time_us, dtype=np.int64)
        assert len(tc) == len(lists)
        ptrs = np.array([s.ctypes.data if len(s) else 0 for s in lists], dtype=np.uint64)
        car, car_p = cls._carry(carry)
        keep = []

        def table(t, n):
            t = {f: np.ascontiguousarray(t[f], dtype=dict(cls.CSMA_FIELDS)[f]) for f in ("status", "attempts", "tick")} if n else {}
            assert all(len(a) == n for a in t.values())
            keep.append(t)
            return _lib.CsmaResult(**{f: a.ctypes.data for f, a in t.items()})
        res, res_c = table(out, int(cnt.sum())), table(carried_out, len(car))
        cap = int(cnt.sum()) + len(car) if cap is None else int(cap)
        got = np.zeros(max(cap, 1), dtype=cls.CSMA_CARRY_DTYPE)
        count = C.c_int64(-1)
        try:
            check(_lib.lib().rm_csma_carry_collect(len(lists), ptrs.ctypes.data, cnt.ctypes.data, tc.ctypes.data, car_p, len(car), C.byref(res),
                                                   C.byref(res_c), got.ctypes.data, cap, C.byref(count)))
        except _lib.RadioMediumError as err:
            err.count = count.value
            raise
        return got[:count.value]

    def csma_carry_collect_device(self, dev_src_ptrs, n_src, cca_time_us, carry, dev_out, dev_carried_out, cap=None):
        """The same from the device form's tables and lists ({field: device pointer}, status / attempts / tick): one compaction on the
        context's stream, one wait.  -> the carry list, a host array."""
        cnt = np.ascontiguousarray(n_src, dtype=np.int32)
        tc = np.ascontiguousarray(cca_time_us, dtype=np.int64)
        ptrs = np.ascontiguousarray([p or 0 for p in dev_src_ptrs], dtype=np.uint64)
        assert len(ptrs) == len(cnt) == len(tc)
        car, car_p = self._carry(carry)
        res, res_c = _lib.CsmaResult(**(dev_out or {})), _lib.CsmaResult(**(dev_carried_out or {}))
        cap = int(cnt.sum()) + len(car) if cap is None else int(cap)
        got = np.zeros(max(cap, 1), dtype=self.CSMA_CARRY_DTYPE)
        count = C.c_int64(-1)
        try:
            check(self._L.rm_csma_carry_collect_device(self._h, len(ptrs), ptrs.ctypes.data, cnt.ctypes.data, tc.ctypes.data, car_p, len(car),
                                                       C.byref(res), C.byref(res_c), got.ctypes.data, cap, C.byref(count)))
        except _lib.RadioMediumError as err:
            err.count = count.value
            raise
        return got[:count.value]

    def sync(self):
        check(self._L.rm_sync(self._h))

    def profile_enable(self, every_n=1):
        check(self._L.rm_profile_enable(self._h, int(every_n)))

    STAGES = ("k_filter", "k_exact", "k_self_entries", "k_cell_off+k_slot_scan", "k_sinr", "k_finalize",
              "k_reorder", "draw kernels", "empty bracket")

    def profile_read(self):
        """-> (sampled ticks, {stage name: summed milliseconds})"""
        n = C.c_uint32()
        ms = (C.c_double * 9)()
        check(self._L.rm_profile_read(self._h, C.byref(n), ms))
        return n.value, {name: ms[i] for i, name in enumerate(self.STAGES)}

    def profile_kernels(self):
        """-> {kernel name as rocprofv3 prints it: (sampled launches, summed milliseconds of the kernel's own dispatch intervals, stage)}"""
        from ._lib import KernelTime
        n = C.c_int32(0)
        buf = (KernelTime * 64)()
        check(self._L.rm_profile_kernels(self._h, buf, 64, C.byref(n)))
        return {buf[i].name.decode(): (buf[i].launches, buf[i].total_ms, self.STAGES[buf[i].stage]) for i in range(min(n.value, 64))}

    def slot_stats(self, slot=0):
        """(candidate links of the sweep's filter, heard links) of result slot `slot`; synchronises"""
        cand, heard = C.c_uint64(0), C.c_uint64(0)
        check(self._L.rm_slot_stats(self._h, slot, C.byref(cand), C.byref(heard)))
        return cand.value, heard.value

    def air_list_stats(self):
        """(ticks that only added their new frames to the on-air lists, ticks that rebuilt the lists) -- SINR extension"""
        inc, reb = C.c_uint64(0), C.c_uint64(0)
        check(self._L.rm_air_list_stats(self._h, C.byref(inc), C.byref(reb)))
        return inc.value, reb.value

    def air_scan_ticks(self):
        """ticks of the SINR extension evaluated by scan: interferers found among the frames on the air, no lists"""
        v = C.c_uint64(0)
        check(self._L.rm_air_scan_ticks(self._h, C.byref(v)))
        return v.value

    def air_batch_stats(self):
        """(batches, ticks) of the SINR extension whose frames outlived their tick and that were swept as batches (rm_airbatch.hip)"""
        b, t = C.c_uint64(0), C.c_uint64(0)
        check(self._L.rm_air_batch_stats(self._h, C.byref(b), C.byref(t)))
        return b.value, t.value

    def air_batch_pairs(self):
        """(pairs evaluated exactly, frames indexed, pairs that interfered) of the last batch of overlapping SINR ticks; synchronises"""
        p, f, i = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(self._L.rm_air_batch_pairs(self._h, C.byref(p), C.byref(f), C.byref(i)))
        return p.value, f.value, i.value

    def air_ring_stats(self):
        """(entries allocated in the busiest sub-ring since the lists were last rebuilt, entries a sub-ring holds)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(self._L.rm_air_ring_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_link_evaluations(self):
        return self._L.rm_last_link_evaluations(self._h)


class Group:
    """n engine contexts behind one caller (rm_group_*): receivers range-partitioned over the members, a tick's Tx
    records handed to every member from the host, results merged in node order."""

    def __init__(self, devices, spatial=True):
        self._L = _lib.lib()
        devs = (C.c_int32 * len(devices))(*devices)
        h = C.c_void_p()
        check(self._L.rm_group_create(len(devices), devs, C.byref(h)))
        self._h = h
        self._n_new = 0
        check(self._L.rm_group_set_partitioning(self._h, 1 if spatial else 0))   # regions of the plane / index ranges

    def close(self):
        if self._h:
            self._L.rm_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return self._L.rm_group_size(self._h)

    def set_model(self, kind, **kw):
        p = Engine.default_params(kind)
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, v)
        check(self._L.rm_group_set_model(self._h, C.byref(p)))

    def seed(self, seed):
        check(self._L.rm_group_seed(self._h, seed))

    @property
    def rng_state(self):
        st = C.c_uint64(0)
        check(self._L.rm_group_get_rng_state(self._h, C.byref(st)))
        return st.value

    def set_link_capacity(self, cap):
        check(self._L.rm_group_set_link_capacity(self._h, cap))

    def upload_table(self, nd):
        def arr(a, dt):
            return np.ascontiguousarray(a, dtype=dt)
        self._keep = [arr(nd.x, np.float64), arr(nd.y, np.float64), arr(nd.z, np.float64), arr(nd.txpower, np.float64),
                      arr(nd.channel, np.int32), arr(nd.enabled, np.uint8), arr(nd.rxprob, np.float64),
                      arr(nd.txprob, np.float64), arr(nd.int_id, np.int32)]
        check(self._L.rm_group_nodes_upload(self._h, nd.n, *[a.ctypes.data for a in self._keep]))
        self._n = nd.n

    def uses_rccl(self):
        rc = self._L.rm_group_uses_rccl(self._h)
        if rc < 0:
            check(rc)
        return bool(rc)

    def tick_run_sources_device(self, t_begin, t_end, dev_src_ptrs, slots, start_us, air_us):
        """the device-resident tick: dev_src_ptrs[r] = `slots` source indices in member r's device memory"""
        ptrs = (C.c_void_p * len(dev_src_ptrs))(*[int(p) for p in dev_src_ptrs])
        check(self._L.rm_group_tick_run_sources_device(self._h, int(t_begin), int(t_end), ptrs, slots, int(start_us), int(air_us)))
        self._n_new = slots * len(dev_src_ptrs)

    def result_copy(self, cap=None):
        n_new = self._n_new
        if cap is None:
            cap = max(1, n_new) * max(1, self._n)
        pkt = np.empty(cap, dtype=np.int32)
        dst = np.empty(cap, dtype=np.int32)
        verdict = np.empty(cap, dtype=np.uint8)
        rssi = np.empty(cap, dtype=np.float64)
        sinr = np.empty(cap, dtype=np.float64)
        pint = np.zeros(max(1, n_new), dtype=np.uint8)
        poff = np.zeros(n_new + 1, dtype=np.uint32)
        cnt = C.c_uint32(0)
        check(self._L.rm_group_result_copy(self._h, pkt.ctypes.data, dst.ctypes.data, verdict.ctypes.data, rssi.ctypes.data,
                                           sinr.ctypes.data, cap, C.byref(cnt), pint.ctypes.data, poff.ctypes.data))
        k = cnt.value
        return TickResult(k, pkt[:k], dst[:k], verdict[:k], rssi[:k], sinr[:k], pint[:n_new], poff)

    def tick(self, recs, t_begin=0, t_end=0, cap=None):
        recs = np.ascontiguousarray(recs, dtype=TX_RECORD_DTYPE)
        n_new = len(recs)
        check(self._L.rm_group_tick_begin(self._h, t_begin, t_end))
        check(self._L.rm_group_enqueue_tx_records(self._h, recs.ctypes.data, n_new))
        if cap is None:
            cap = max(1, n_new) * max(1, self._n)
        pkt = np.empty(cap, dtype=np.int32)
        dst = np.empty(cap, dtype=np.int32)
        verdict = np.empty(cap, dtype=np.uint8)
        rssi = np.empty(cap, dtype=np.float64)
        sinr = np.empty(cap, dtype=np.float64)
        pint = np.zeros(max(1, n_new), dtype=np.uint8)
        poff = np.zeros(n_new + 1, dtype=np.uint32)
        cnt = C.c_uint32(0)
        check(self._L.rm_group_tick_flush(self._h, pkt.ctypes.data, dst.ctypes.data, verdict.ctypes.data, rssi.ctypes.data,
                                          sinr.ctypes.data, cap, C.byref(cnt), pint.ctypes.data, poff.ctypes.data))
        k = cnt.value
        return TickResult(k, pkt[:k], dst[:k], verdict[:k], rssi[:k], sinr[:k], pint[:n_new], poff)
