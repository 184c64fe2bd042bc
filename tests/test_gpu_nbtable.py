"""The neighbour tables (rm_nbtable_*, rm_nbtable.hip) on the GPU.  The scenes are those of
tests/nbtable_ref.py, played by a driver that sends every call to the engine as well: ticks are the engine's, the reference is moved
from the result copied out of the engine by rm_result_copy, and after EVERY call the whole peer table, every rm_link_stats entry,
the watched links' totals, the node counters and the totals are compared with the reference -- exactly.  Host and device forms are
used in turn.  tests/test_nbtable_ref.py holds the scenes' conditions for the reference alone."""
import ctypes as C

import numpy as np
import pytest

import linkstats_ref as LS
import nbtable_ref as R
from test_gpu_fwd import launches_added
from util import DeviceArray, KINDS, _PARAM_MAP

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5


def same_state(eng, ref, what):
    """both of E14's tables, its totals, the counters and the totals against the reference"""
    np.testing.assert_array_equal(eng.linkstats_peers(), ref.tab.peer, err_msg=what + ": peer")
    stats, lt = eng.linkstats_read()
    LS.equal(stats, ref.tab, what)
    assert lt == ref.tab.totals(), (what, lt, ref.tab.totals())
    rows, tot = eng.nbtable_read()
    for f in R.NODE_FIELDS:
        assert rows[f].tolist() == ref.cnt[f], (what, f)
    assert not rows["reserved"].any() and tot == ref.totals(), (what, tot, ref.totals())
    return rows, tot


class GpuDriver(R.Driver):
    """every call to the engine and to the reference; ticks are the engine's"""

    def __init__(self, rsa, nd, kind, params, K, listen=None, errmodel=None, **nbt):
        super().__init__(nd, kind, params, K, listen, errmodel, **nbt)
        self.rsa = rsa
        self.eng = rsa.Engine(0)
        self.eng.upload_table(nd)
        self.eng.set_model(KINDS[kind], **{_PARAM_MAP[k]: v for k, v in params.items()})
        if errmodel is not None:
            self.eng.set_error_model(rsa._lib.EM_OQPSK_250K, seed=errmodel)
        if listen is not None:
            self.eng.listen_set(np.asarray(listen, dtype=np.int64))
        self.eng.linkstats_enable(K)
        self.eng.nbtable_enable(**nbt)
        self.bufs, self.calls = [], 0

    def dev(self, a):
        d = DeviceArray(np.ascontiguousarray(a))
        self.bufs.append(d)
        return d

    def close(self):
        for d in self.bufs:
            d.free()
        self.eng.close()

    def after(self, what):
        super().after(what)
        self.calls += 1
        same_state(self.eng, self.ref, "%s (call %d)" % (what, self.calls))

    # -- ticks: the engine's, copied out
    def set_capacity(self, cap):
        super().set_capacity(cap)
        self.eng.set_link_capacity(cap)

    def _copied(self, src, copy, start, dropped):
        """copy(): the engine's result; a slot over the link capacity has none to copy (rm_result_copy refuses) and is lost"""
        if dropped:
            return self.result(src, start, [0] * (len(src) + 1), [], [], [], [], True)
        r = copy()
        return self.result(src, start, r.pkt_offset, r.dst, r.verdict, r.rssi, r.sinr)

    def tick(self, t_begin, t_end, src, start, air):
        d = self.dev(np.asarray(src, dtype=np.int32))
        self.eng.tick_run_sources_device(t_begin, t_end, d.ptr.value, len(src), start, air)
        res = self._copied(src, lambda: self.eng.result_copy(len(src)), start, self.eng.result_count()[1])
        self.ref.count(res)
        return res

    def batch(self, t_begin, t_end, lists, starts, air):
        ds = [self.dev(np.asarray(l, dtype=np.int32)) for l in lists]
        self.eng.batch_run_sources_device(t_begin, t_end, [d.ptr.value for d in ds], [len(l) for l in lists], starts, [air] * len(lists))
        out = [self._copied(l, lambda: self.eng.batch_result_copy(b, len(l)), starts[b], self.eng.batch_result_count(b)[1]) for b, l in enumerate(lists)]
        for res in out:
            self.ref.count(res)
        return out

    # -- the calls: host and device forms in turn
    def _pin(self, pin):
        return None if pin is None else self.dev(np.asarray(pin, dtype=np.int32)).ptr.value

    def update(self, res, time_us, pin=None, slot=0):
        if self.calls % 2:
            self.eng.nbtable_update_device(slot, time_us, self._pin(pin))
        else:
            self.eng.nbtable_update(slot, time_us, pin)
        super().update(res, time_us, pin, slot)

    def expire(self, time_us, pin=None):
        if self.calls % 2:
            self.eng.nbtable_expire(time_us, pin)
        else:
            self.eng.nbtable_expire_device(time_us, self._pin(pin))
        super().expire(time_us, pin)

    def watch(self, nodes, rows):
        self.eng.linkstats_watch(rows, nodes)
        super().watch(nodes, rows)

    def stats_reset(self):
        self.eng.linkstats_reset()
        super().stats_reset()

    def reset(self):
        self.eng.nbtable_reset()
        super().reset()


@pytest.fixture()
def make(rsa):
    made = []

    def _make(*a, **kw):
        made.append(GpuDriver(rsa, *a, **kw))
        return made[-1]
    yield _make
    for d in made:
        d.close()


# ---- the scenes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("shape", ["line", "clique"])
def test_tables_from_empty(O, make, shape, n, K):
    d = R.scene_fill(make, shape, n, K)
    _, tot = d.eng.nbtable_read()
    assert tot["updates"] == 8 and tot["admitted"] >= n and (tot["refused"] > 0) == (K < 8)


def test_tie_goes_to_the_least_source(O, make):
    d = R.scene_tie(make)
    assert d.eng.linkstats_peers()[0].tolist() == [1]


def test_long_bid_pass(O, make):
    """96 transmitters of a 192-node clique: 18 336 links, more than one stride of the bid and count passes"""
    d = R.scene_long(make)
    assert d.ref.log["bids"] >= 18336 and d.eng.nbtable_read()[1]["admitted"] == 2 * 192


@pytest.mark.parametrize("n", [1025, 4097])
def test_several_workgroups(O, make, n):
    d = R.scene_big(make, n)
    tot = d.eng.nbtable_read()[1]
    assert tot["admitted"] > n // 2 and tot["expired"] > n // 8


@pytest.mark.parametrize("require_delivered", [0, 1])
def test_media(O, make, require_delivered):
    """33 x 33 on the SINR medium with E13's schedules and E10's model: collided and missed copies, bids heard but not delivered"""
    d = R.scene_media(make, require_delivered)
    assert d.ref.log["undelivered_bidders"] >= 10 and d.ref.log["low"] >= 10 and d.ref.log["ties"] >= 1
    assert (d.ref.log["undelivered_admitted"] >= 1) == (require_delivered == 0)
    assert int(d.eng.listen_missed().sum()) >= 1


def test_evictions_and_pins(O, make):
    d = R.scene_evict(make)
    assert d.eng.linkstats_peers()[0].tolist() == [3, 2] and d.ref.log["stale_choice"] >= 1
    d = R.scene_poor(make)
    assert d.ref.log["poor_zero_first"] >= 1 and d.ref.log["refused_pinned"] >= 1 and d.eng.nbtable_read()[1]["evicted_poor"] >= 1
    d = R.scene_pins(make)
    assert d.ref.log["refused_pinned"] >= 3 and d.eng.linkstats_peers()[4].tolist() == [2] and d.eng.nbtable_read()[1]["expired"] == 0
    d = R.scene_disabled(make)
    tot = d.eng.nbtable_read()[1]
    assert tot["expired"] == 0 and tot["evicted_stale"] == tot["evicted_poor"] == 0 and tot["refused"] >= 8


def test_device_pin_entries_outside_the_table_pin_nothing(O, make):
    """the device form takes any int32: entries at or above the node count and negative ones pin nothing, so the stale slot goes"""
    n = 5
    d = make(R.clique_nodes(n, 5.0), "udgm", R.UDGM, 1, timeout_us=3 * R.TICK, evict_cost=0)
    t = R.rounds(d, [[0], [1]])       # (t < timeout_us at both updates: nobody is stale, node 1's frame is refused by the full rows)
    assert d.eng.linkstats_peers()[:, 0].tolist() == [1, 0, 0, 0, 0]
    pin = np.array([n, n + 7, 2 ** 31 - 1, -(2 ** 31), -1], dtype=np.int32)
    res = d.tick(t + 4 * R.TICK, t + 5 * R.TICK, [2], t + 4 * R.TICK + 100, R.AIR)
    d.calls |= 1                      # (the device form of update)
    d.update(res, t + 5 * R.TICK, pin)
    assert d.eng.linkstats_peers()[:, 0].tolist() == [2, 2, 0, 2, 2] and d.eng.nbtable_read()[1]["evicted_stale"] == 4
    d.calls &= ~1                     # (the device form of expire)
    d.expire(t + 50 * R.TICK, pin)
    assert (d.eng.linkstats_peers() == -1).all()


def test_lost_slot_and_small_scenes(O, make):
    d = R.scene_capacity(make)
    assert d.unchanged and d.eng.nbtable_read()[1]["skipped_slots"] == 1
    d = R.scene_dup(make)
    assert d.ref.log["dup_counted"] == 3 and (d.eng.linkstats_read()[0]["heard"][[0, 2, 3], 0] == 2).all()
    d = R.scene_weak(make)
    assert d.ref.log["low"] >= 8


def test_batch(O, make):
    """8 ticks in one rm_batch_run_sources_device with an update per slot in ascending order, and 8 lone ticks with an update each:
    each equals the host rule in its order (compared after every call), the peers agree and the counters differ"""
    a, b = R.scene_batch(make, True), R.scene_batch(make, False)
    sa, sb = a.eng.linkstats_read()[0], b.eng.linkstats_read()[0]
    assert a.eng.linkstats_peers().tobytes() == b.eng.linkstats_peers().tobytes()
    assert (sa["heard"] != sb["heard"]).any() and (sa["heard"] <= sb["heard"]).all()


def test_reset_and_linkstats_reset(O, make):
    """rm_nbtable_reset zeroes the counters and leaves E14's tables; rm_linkstats_reset makes every entry stale"""
    d = R.scene_fill(make, "clique", 64, 2)
    d.reset()
    assert not any(d.eng.nbtable_read()[1].values()) and (d.eng.linkstats_peers() >= 0).all()
    d2 = make(R.clique_nodes(6, 5.0), "udgm", R.UDGM, 2, timeout_us=1 << 30, evict_cost=0)
    t = R.rounds(d2, [[0], [1]])
    d2.stats_reset()
    d2.expire(t)
    assert (d2.eng.linkstats_peers() == -1).all() and d2.eng.nbtable_read()[1]["expired"] == 10


# ---- the chain: beacons -> discovery -> counters -> routes -> forwarding, from an empty watch table --------------------------------

CHAIN_STEPS, CHAIN_TAIL, ROOT, QUIET = 25, 15, 40, 0
CHAIN = dict(timeout_us=7 * R.TICK, evict_cost=0)


def _chain_setup(d):
    """E15 beacons, one every five ticks, in the tick (x + 2 y) mod 5: a node's four neighbours send in four different ticks"""
    n = d.nd.n
    sched = np.array([(5 * R.TICK, ((j % 9 + 2 * (j // 9)) % 5) * R.TICK + 50, 0, 0) for j in range(n)], dtype=np.int64)
    d.eng.traffic_set(sched)
    d.eng.fwd_enable(queue_slots=4)
    return sched


def _silence(d, sched):
    row = sched[QUIET:QUIET + 1].copy()
    row[:] = 0
    d.eng.traffic_set(row, nodes=[QUIET])


def _chain_device(rsa):
    """everything on the device, nothing read in between -> the final tables' bytes, the query's totals"""
    nd = R.lattice_nodes()
    n = nd.n
    d = GpuDriver(rsa, nd, "logdist", R.LATTICE, 4, **CHAIN)
    try:
        eng = d.eng
        sched = _chain_setup(d)
        P = eng.etx_params(min_heard=1)
        d_src, d_count = d.dev(np.full(n, -1, dtype=np.int32)), d.dev(np.zeros(1, dtype=np.int32))
        d_parent, d_cost, d_roots = d.dev(np.full(n, -1, dtype=np.int32)), d.dev(np.zeros(n, dtype=np.uint64)), d.dev(np.array([ROOT], dtype=np.int32))
        tot = None
        for k in range(CHAIN_STEPS + CHAIN_TAIL):
            t = k * R.TICK
            if k == CHAIN_STEPS:
                _silence(d, sched)
            eng.traffic_generate_device(5, [t], [t + R.TICK], n, d_src.ptr.value, d_count.ptr.value)
            eng.tick_run_sources_device(t, t + R.TICK, d_src.ptr.value, n, t + 100, R.AIR)
            eng.nbtable_update_device(0, t + R.TICK, d_parent.ptr.value)
            if k % 5 == 4:
                tot = eng.etx_routes_device(P, d_roots.ptr.value, 1, d_cost.ptr.value, d_parent.ptr.value, dev_cur_ptr=d_parent.ptr.value)
                eng.fwd_set_next_device(d_parent.ptr.value, d_roots.ptr.value, 1, t + R.TICK)
        eng.nbtable_expire_device((CHAIN_STEPS + CHAIN_TAIL) * R.TICK, d_parent.ptr.value)
        rows, nt = eng.nbtable_read()
        return eng.linkstats_peers(), eng.linkstats_read()[0], rows, nt, tot, eng.fwd_read()[0]["next"].copy()
    finally:
        d.close()


def test_chain(rsa, O, make):
    """from an all-empty watch table on the 9 x 9 lattice: the device run twice gives the same bytes, and they are those of the
    stepwise run that is compared with the reference after every call; every node is reached, and the expire after silencing a
    corner node removes it from its neighbours' rows"""
    a, b = _chain_device(rsa), _chain_device(rsa)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3] == b[3] and a[4] == b[4]
    nd = R.lattice_nodes()
    n = nd.n
    d = make(nd, "logdist", R.LATTICE, 4, **CHAIN)
    eng = d.eng
    sched = _chain_setup(d)
    P = eng.etx_params(min_heard=1)
    parents = np.full(n, -1, dtype=np.int32)
    before = None
    for k in range(CHAIN_STEPS + CHAIN_TAIL):
        t = k * R.TICK
        if k == CHAIN_STEPS:
            _silence(d, sched)
            before = eng.linkstats_peers()
        rows, count, _ = eng.traffic_generate(5, [t], [t + R.TICK], n)
        assert (QUIET in rows[0].tolist()) == (k % 5 == 0 and k < CHAIN_STEPS)
        d.calls |= 1              # (the device form, as in the device run)
        d.update(d.tick(t, t + R.TICK, rows[0].tolist(), t + 100, R.AIR), t + R.TICK, parents)
        if k % 5 == 4:
            out, tot = eng.etx_routes(P, [ROOT], cur=parents)
            parents = out["parent"].astype(np.int32)
    d.calls &= ~1
    d.expire((CHAIN_STEPS + CHAIN_TAIL) * R.TICK, parents)
    peers, stats = eng.linkstats_peers(), eng.linkstats_read()[0]
    rows, nt = eng.nbtable_read()
    assert a[0].tobytes() == peers.tobytes() and a[1].tobytes() == stats.tobytes() and a[2].tobytes() == rows.tobytes() and a[3] == nt
    assert a[4] == tot and tot["reached"] == n and a[5][ROOT] == -2 and (np.delete(a[5], ROOT) >= 0).all()
    assert (before[[1, 9]] == QUIET).any(axis=1).all() and not (peers == QUIET).any() and nt["expired"] >= 2
    assert (peers[QUIET] >= 0).sum() == 2           # (the silent node still hears its two neighbours)


# ---- launches per call; off by default ----------------------------------------------------------------------------------------------

def _lattice_engine(rsa, nd):
    eng = rsa.Engine(0)
    eng.upload_table(nd)
    eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in R.LATTICE.items()})
    eng.profile_enable(1)
    return eng


def test_launches_per_call(rsa, O):
    """an update is four launches and an expire one, each kernel under its name once"""
    nd = R.lattice_nodes()
    eng = _lattice_engine(rsa, nd)
    src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
    try:
        eng.linkstats_enable(4)
        eng.nbtable_enable()
        eng.tick_run_sources_device(0, R.TICK, src.ptr.value, 27, 100, R.AIR)
        added = launches_added(eng, "k_nbt_", lambda: eng.nbtable_update(0, R.TICK))
        assert added == {"k_nbt_bid": 1, "k_nbt_settle": 1, "k_nbt_count": 1, "k_nbt_rest": 1}, added
        added = launches_added(eng, "k_nbt_", lambda: eng.nbtable_expire(R.TICK))
        assert added == {"k_nbt_expire": 1}, added
        assert eng.nbtable_read()[1]["admitted"] >= 1
    finally:
        src.free()
        eng.close()


def test_update_without_a_result_and_off_by_default(rsa, O):
    """no evaluated result yet: STATE.  Off by default: a plain run launches no k_nbt_* kernel, and an existing call's results and
    E14's tables are the same with the feature on and never called"""
    nd = R.lattice_nodes()
    outs = []
    for on in (False, True):
        eng = _lattice_engine(rsa, nd)
        try:
            eng.linkstats_enable(2)
            assert not eng.nbtable_enabled()
            if on:
                eng.nbtable_enable()
                assert _code(rsa, lambda: eng.nbtable_update(0, 0)) == STATE
                assert _code(rsa, lambda: eng.nbtable_update_device(0, 0, None)) == STATE
            src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
            try:
                eng.tick_run_sources_device(0, R.TICK, src.ptr.value, 27, 100, R.AIR)
                r = eng.result_copy(27)
            finally:
                src.free()
            outs.append((r.count, r.pkt.tobytes(), r.dst.tobytes(), r.verdict.tobytes(), r.rssi.tobytes(), r.sinr.tobytes(), r.pkt_offset.tobytes(),
                         eng.linkstats_peers().tobytes(), eng.linkstats_read()[0].tobytes()))
            if on:
                eng.nbtable_update(0, R.TICK)
                assert eng.nbtable_read()[1]["admitted"] >= 1
            names = [k for k in eng.profile_kernels() if k.startswith("k_nbt_")]
            assert bool(names) == on, names
        finally:
            eng.close()
    assert outs[0] == outs[1]


# ---- refusals and lifetime ----------------------------------------------------------------------------------------------------------

def _code(rsa, call):
    with pytest.raises(rsa.RadioMediumError) as e:
        call()
    return e.value.code


def test_refusals_leave_the_state_unchanged(rsa, O, make):
    d = R.scene_fill(make, "clique", 65, 2)      # (tables with history, and an evaluated result)
    eng, n = d.eng, d.nd.n
    L, h = eng._L, eng._h
    pin = np.full(n, -1, dtype=np.int32)
    big = pin.copy()
    big[7] = n
    out = np.zeros(n, dtype=eng.nbtable_read()[0].dtype)
    dv = d.dev(pin)
    # INVALID: NULL arguments, negative times, a slot outside the last call's, a host pin entry >= n_nodes, bad lists
    calls = [lambda: L.rm_nbtable_update(h, 0, -1, None), lambda: L.rm_nbtable_update(h, 1, 0, None), lambda: L.rm_nbtable_update(h, -1, 0, None),
             lambda: L.rm_nbtable_update(h, 0, 0, big.ctypes.data), lambda: L.rm_nbtable_update_device(h, 0, -5, dv.ptr.value),
             lambda: L.rm_nbtable_update_device(h, 7, 0, None), lambda: L.rm_nbtable_update(None, 0, 0, None),
             lambda: L.rm_nbtable_expire(h, -1, None), lambda: L.rm_nbtable_expire(h, 0, big.ctypes.data), lambda: L.rm_nbtable_expire_device(h, -1, None),
             lambda: L.rm_nbtable_expire(None, 0, None), lambda: L.rm_nbtable_read(h, None, 3, None, None),
             lambda: L.rm_nbtable_read(h, pin.ctypes.data, -1, None, None),
             lambda: L.rm_nbtable_read(h, np.array([n], dtype=np.int32).ctypes.data, 1, out.ctypes.data, None),
             lambda: L.rm_nbtable_enable(h, None), lambda: L.rm_nbtable_enable(None, C.byref(eng.nbtable_params())),
             lambda: L.rm_nbtable_get_params(h, None), lambda: L.rm_nbtable_device(None, None, None), lambda: L.rm_nbtable_reset(None)]
    for k, call in enumerate(calls):
        assert call() == INVALID, k
    for kw in (dict(admit_rssi_dbm=float("nan")), dict(timeout_us=-1), dict(min_heard=(1 << 31) + 1), dict(evict_cost=100), dict(require_delivered=2),
               dict(reserved=1)):
        bad = eng.nbtable_params(**kw)
        assert _code(rsa, lambda: eng.nbtable_enable(bad)) == INVALID and eng.nbtable_enabled()
    same_state(eng, d.ref, "after the INVALID refusals")
    # STATE: a receiver partition
    eng.set_partition(0, n // 2)
    assert _code(rsa, lambda: eng.nbtable_update(0, 0)) == STATE
    eng.set_partition(0, n)
    same_state(eng, d.ref, "after the STATE refusal")
    # the same node count, rm_node_update, rm_nodes_move and the same K keep everything
    eng.upload_table(d.nd)
    eng.update_node(1, 1.0, 0.0, 0.0, 0.0, int(d.nd.channel[1]), 1, 1.0, 1.0)
    eng.move_nodes([2, 3], [0.5, 1.5], [0.0, 0.0])
    eng.linkstats_enable(2)
    assert eng.nbtable_enabled()
    same_state(eng, d.ref, "after an upload of the same node count, a move and the same K")
    assert eng.nbtable_get_params().min_heard == 4 and all(p for p in eng.nbtable_device())
    # off: every call but enable / enabled / disable is refused; enable again starts the counters from nothing, E14's tables stay
    peers = eng.linkstats_peers()
    eng.nbtable_disable()
    assert not eng.nbtable_enabled()
    for call in (lambda: eng.nbtable_update(0, 0), lambda: eng.nbtable_update_device(0, 0, None), lambda: eng.nbtable_expire(0),
                 lambda: eng.nbtable_expire_device(0, None), lambda: eng.nbtable_read(), lambda: eng.nbtable_reset(), lambda: eng.nbtable_device(),
                 lambda: eng.nbtable_get_params()):
        assert _code(rsa, call) == STATE
    eng.nbtable_enable(min_heard=9)
    rows, tot = eng.nbtable_read()
    assert not rows["admitted"].any() and not any(tot.values()) and eng.nbtable_get_params().min_heard == 9
    assert eng.linkstats_peers().tobytes() == peers.tobytes()
    # another K switches the feature off with E14's tables; E14 off: enable is refused
    eng.linkstats_enable(4)
    assert not eng.nbtable_enabled() and _code(rsa, lambda: eng.nbtable_update(0, 0)) == STATE
    eng.linkstats_enable(0)
    assert _code(rsa, lambda: eng.nbtable_enable()) == STATE and not eng.nbtable_enabled()
    # another node count switches both off
    eng.linkstats_enable(2)
    eng.nbtable_enable()
    eng.upload_table(R.line_nodes(n + 1))
    assert not eng.nbtable_enabled() and eng.linkstats_enabled() == 0


def test_update_after_a_gathered_form_is_refused(rsa, O):
    """the last evaluating call was a gathered form (rm_dist_* and rm_group_* leave the same mark): STATE, nothing changes; a lone
    tick after it is taken again"""
    nd = R.lattice_nodes()       # (81 nodes: a sorted receiver table, which the gathered forms need)
    eng = rsa.Engine(0)
    dv = DeviceArray(np.array([1, 31, 61], dtype=np.int32))
    try:
        eng.upload_table(nd)
        eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in R.N.PLAIN.items()})
        # (E14 refuses the gathered forms while it is on: the statistics and this feature are switched on behind the call)
        eng.batch_run_gathered_sources_device([R.TICK], [2 * R.TICK], dv.ptr.value, 1, 3, [R.TICK + 100], R.AIR)
        eng.linkstats_enable(4)
        eng.nbtable_enable(**R.FILL)
        assert _code(rsa, lambda: eng.nbtable_update(0, 2 * R.TICK)) == STATE
        assert _code(rsa, lambda: eng.nbtable_update_device(0, 2 * R.TICK, None)) == STATE
        eng.nbtable_expire(0)         # (no result slot is read: accepted)
        assert not any(eng.nbtable_read()[1].values()) and (eng.linkstats_peers() == -1).all()
        eng.tick_run_sources_device(4 * R.TICK, 5 * R.TICK, dv.ptr.value, 3, 4 * R.TICK + 100, R.AIR)
        eng.nbtable_update(0, 5 * R.TICK)
        assert eng.nbtable_read()[1]["admitted"] >= 6
    finally:
        dv.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import radio_sim_amd as rsa
import nbtable_ref as R
eng = rsa.Engine(0)
eng.upload_table(R.line_nodes(8))
for call in (lambda: eng.linkstats_enable(2), lambda: eng.nbtable_enable(), lambda: eng.nbtable_update(0, 0), lambda: eng.nbtable_expire(0)):
    try:
        call()
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        print("REFUSED", "RM_GRAPH" in str(e))
    else:
        print("ACCEPTED")
print(int(eng.nbtable_enabled()))
eng.close()
"""


def test_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- takes none of the extensions: enable is refused and names the
    knob, and so every other call finds the feature off"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % (root, root)], cwd=root, env=dict(os.environ, RM_GRAPH="1"), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.split() == ["REFUSED", "True", "REFUSED", "True", "REFUSED", "False", "REFUSED", "False", "0"], p.stdout


def test_enable_without_nodes_is_refused(rsa):
    eng = rsa.Engine(0)
    try:
        eng.linkstats_enable(2)
        assert _code(rsa, lambda: eng.nbtable_enable()) == STATE and not eng.nbtable_enabled()
        assert _code(rsa, lambda: eng.nbtable_get_params()) == STATE
        eng.upload_table(R.line_nodes(3))
        assert eng.linkstats_enabled() == 0             # (another node count switched E14 off)
        assert _code(rsa, lambda: eng.nbtable_enable()) == STATE
        eng.linkstats_enable(2)
        eng.nbtable_enable(timeout_us=0)
        assert eng.nbtable_get_params().timeout_us == 0 and eng.nbtable_read()[0].shape == (3,)
    finally:
        eng.close()
