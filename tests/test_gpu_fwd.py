"""The forwarding queues (rm_fwd_*, rm_fwd.hip) on the GPU.  The scenes are those of tests/fwd_ref.py, played
by a driver that sends every call to the engine as well: ticks are the engine's, the reference is advanced from the result copied out
of the engine by rm_result_copy, and after EVERY step the whole node table, the totals, every queue in queue order and the source
lists are compared with the reference -- exactly.  tests/test_fwd_ref.py holds the scenes' conditions for the reference alone."""
import ctypes as C

import numpy as np
import pytest

import fwd_ref as F
import hops_ref as H
from test_gpu_traffic import MULTI_ROUND, _bare, _chunk
from util import DeviceArray, KINDS, _PARAM_MAP

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5


def same_state(eng, ref, what):
    """the whole table, the totals and every queue in queue order, against the reference"""
    rows, tot = eng.fwd_read()
    want = ref.table()
    for f in F.NODE_FIELDS:
        np.testing.assert_array_equal(rows[f].astype(object), np.array(want[f], dtype=object), err_msg="%s: %s" % (what, f))
    assert not rows["slot_mask"].any() and not rows["reserved"].any(), what
    assert tot == ref.totals(), (what, tot, ref.totals())
    pk, ln = eng.fwd_queue_read()
    q = ref.queues()
    np.testing.assert_array_equal(ln, [len(v) for v in q], err_msg=what + ": queue lengths")
    got = [[tuple(int(x) for x in pk[j][s]) for s in range(int(ln[j]))] for j in range(ref.n)]
    assert got == q, what
    unused = np.arange(pk.shape[1])[None, :] >= ln[:, None]
    assert not any(pk[f][unused].any() for f in pk.dtype.names), what + ": unused entries"
    return rows, tot


class GpuDriver(F.Driver):
    """every call to the engine and to the reference; ticks are the engine's"""

    def __init__(self, rsa, nd, kind, params, **fwd):
        super().__init__(nd, kind, params, **fwd)
        self.rsa = rsa
        self.eng = rsa.Engine(0)
        self.eng.upload_table(nd)
        self.eng.set_model(KINDS[kind], **{_PARAM_MAP[k]: v for k, v in params.items()})
        self.eng.fwd_enable(**fwd)
        self.bufs, self.calls, self.dev_tree = [], 0, None
        self.d_src = self.dev(np.full(max(nd.n, 1) + 8, -1, dtype=np.int32))
        self.d_count = self.dev(np.zeros(1, dtype=np.int32))

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

    # -- routes: the hop query's parent array and root list as they lie in device memory
    def tree(self, roots):
        n = self.nd.n
        self.dev_tree = (self.dev(np.zeros(n, dtype=np.int32)), self.dev(np.zeros(n, dtype=np.int32)), self.dev(np.asarray(roots, dtype=np.int32)))
        hop, par, dr = self.dev_tree
        self.eng.hops_device(H.HEARD_BY, dr.ptr.value, len(roots), hop.ptr.value, par.ptr.value)
        self.tree_parent = super().tree(roots)
        return self.tree_parent

    def set_next(self, parent, roots, time_us):
        if self.dev_tree is not None and parent is self.tree_parent:
            self.eng.fwd_set_next_device(self.dev_tree[1].ptr.value, self.dev_tree[2].ptr.value, len(roots), time_us)
        else:
            self.eng.fwd_set_next(parent, roots, time_us)
        super().set_next(parent, roots, time_us)

    def inject(self, src, time_us):
        if self.calls % 2:
            d = self.dev(np.asarray(src, dtype=np.int32))
            self.eng.fwd_inject_device(d.ptr.value, len(src), time_us)
        else:
            self.eng.fwd_inject(src, time_us)
        super().inject(src, time_us)

    def set_traffic(self, table, seed):
        super().set_traffic(table, seed)
        self.eng.traffic_set(np.asarray(table, dtype=np.int64))
        self.d_row = self.dev(np.zeros(self.nd.n, dtype=np.int32))
        self.d_row_count = self.dev(np.zeros(1, dtype=np.int32))

    def inject_traffic(self, lo, hi):
        """E15's row, whole (n = cap), from device memory"""
        self.eng.traffic_generate_device(self.traffic[1], [lo], [hi], self.nd.n, self.d_row.ptr.value, self.d_row_count.ptr.value)
        self.eng.fwd_inject_device(self.d_row.ptr.value, self.nd.n, lo)
        super().inject_traffic(lo, hi)

    def sources(self, time_us, cap):
        want, count = super().sources(time_us, cap)
        got, n = self.eng.fwd_sources(time_us, cap)
        assert (got.tolist(), n) == (want, count), ("sources", time_us, cap)
        assert cap <= self.nd.n + 8
        self.eng.fwd_sources_device(time_us, cap, self.d_src.ptr.value, self.d_count.ptr.value)
        assert DeviceArray.read(self.d_src.ptr.value, np.int32, cap).tolist() == want
        assert int(DeviceArray.read(self.d_count.ptr.value, np.int32, 1)[0]) == count
        return want, count

    # -- ticks: the engine's, copied out
    def _copied(self, src, r, start, air):
        return F.records_result(self.nd.n, src, start, air, r.pkt_offset, r.dst, r.verdict)

    def tick(self, t_begin, t_end, src, start, air):
        d = self.dev(np.asarray(src, dtype=np.int32))
        self.eng.tick_run_sources_device(t_begin, t_end, d.ptr.value, len(src), start, air)
        return self._copied(src, self.eng.result_copy(len(src)), start, air)

    def tick_cca(self, t_begin, t_end, src, start, air, cca_time, threshold):
        flags, _ = self.eng.tick_run_sources_cca(t_begin, t_end, src, start, air, cca_time, threshold)
        kept = np.where(flags != 0, -1, np.asarray(src, dtype=np.int32))
        return self._copied(kept, self.eng.result_copy(len(src)), start, air)

    def batch(self, t_begin, t_end, lists, starts, air):
        ds = [self.dev(np.asarray(l, dtype=np.int32)) for l in lists]
        self.eng.batch_run_sources_device(t_begin, t_end, [d.ptr.value for d in ds], [len(l) for l in lists], starts, [air] * len(lists))
        return [self._copied(l, self.eng.batch_result_copy(b, len(l)), starts[b], air) for b, l in enumerate(lists)]

    def advance(self, res, cand=None, slot=0):
        if cand is not None and self.calls % 2:
            d = self.dev(np.asarray(cand, dtype=np.int32))
            self.eng.fwd_advance_device(slot, d.ptr.value, len(cand))
        else:
            self.eng.fwd_advance(slot, cand)
        super().advance(res, cand, slot)

    def reset(self):
        self.eng.fwd_reset()
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

@pytest.mark.parametrize("n", [40, 70])
def test_line(O, make, n):
    """40: the whole-table scan; 70: boxes.  Every packet arrives with hops = its distance"""
    d = F.scene_line(make, n)
    rows, tot = d.eng.fwd_read()
    assert tot["arrived"] == n and rows["hops_sum"].tolist() == list(range(n))


@pytest.mark.parametrize("leaves", [64, 65, 129, 257])
def test_hub_sink(O, make, leaves):
    d = F.scene_hub_sink(make, leaves)
    assert d.eng.fwd_read()[1]["arrived"] == leaves


@pytest.mark.parametrize("arrivals, preload", [(16, 0), (17, 0), (15, 1), (16, 1)])
def test_hub_relay(O, make, arrivals, preload):
    d = F.scene_hub_relay(make, arrivals, preload)
    rows, _ = d.eng.fwd_read([20])
    assert int(rows["rejected"][0]) == (0 if preload + arrivals <= 16 else arrivals)


@pytest.mark.parametrize("retries, min_be, max_be", [(0, 0, 0), (3, 0, 0), (0, 3, 5), (3, 3, 5)])
def test_lattice(O, make, retries, min_be, max_be):
    """next from rm_hops_query_device as it lies in device memory, E15's rows from device memory, 200 plain lone ticks"""
    d = F.scene_lattice(make, retries, min_be, max_be)
    assert d.log["steps"] == 200 and d.eng.fwd_read()[1]["arrived"] >= 5


@pytest.mark.parametrize("cand", [True, False])
def test_gated(O, make, cand):
    d = F.scene_lattice(make, 3, 3, 5, steps=120, cca=(128, -88.0), cand=cand)
    rows, _ = d.eng.fwd_read()
    assert d.log["deferred_lists"] >= 1 and (int(rows["deferred"].sum()) >= 1) == cand


@pytest.mark.parametrize("n", [1025, 4097])
def test_big(O, make, n):
    d = F.scene_big(make, n)
    assert d.log["truncated"] >= 2


def test_reroute(O, make):
    d = F.scene_reroute(make)
    _, tot = d.eng.fwd_read()
    assert (tot["dropped_no_route"], tot["dropped_ttl"], tot["in_flight"]) == (3, 2, 0)


def test_batch(O, make):
    """8 node-disjoint ticks in one rm_batch_run_sources_device, an advance per slot: the state of 8 lone ticks with an advance each"""
    a, b = F.scene_batch(make, True), F.scene_batch(make, False)
    ra, ta = a.eng.fwd_read()
    rb, tb = b.eng.fwd_read()
    assert ra.tobytes() == rb.tobytes() and ta == tb and ta["stray"] >= 1
    qa, qb = a.eng.fwd_queue_read(), b.eng.fwd_queue_read()
    assert qa[0].tobytes() == qb[0].tobytes() and qa[1].tolist() == qb[1].tolist()


def _chain(rsa, steps=50):
    """inject -> sources -> tick with n = cap -> advance, on the device, nothing read in between -> the final state's bytes"""
    nd = F.lattice_nodes()
    n = nd.n
    d = GpuDriver(rsa, nd, "logdist", F.LATTICE, queue_slots=4, max_retries=3, min_be=3, max_be=5, backoff_unit_us=1000, seed=11)
    try:
        eng = d.eng
        d.set_next(d.tree([0]), [0], 0)
        table = F.lattice_table(n, 0)
        eng.traffic_set(np.asarray(table, dtype=np.int64))
        lo = [k * F.TICK for k in range(steps)]
        rows = d.dev(np.zeros(steps * n, dtype=np.int32))
        counts = d.dev(np.zeros(steps, dtype=np.int32))
        eng.traffic_generate_device(5, lo, [t + F.TICK for t in lo], n, rows.ptr.value, counts.ptr.value)
        for k, t in enumerate(lo):
            eng.fwd_inject_device(rows.ptr.value + 4 * k * n, n, t)
            eng.fwd_sources_device(t + 100, n, d.d_src.ptr.value, d.d_count.ptr.value)
            eng.tick_run_sources_device(t, t + F.TICK, d.d_src.ptr.value, n, t + 100, F.AIR)
            eng.fwd_advance_device(0, None, 0)
        r, tot = eng.fwd_read()
        pk, ln = eng.fwd_queue_read()
        return r, tot, pk, ln
    finally:
        d.close()


def test_chain(rsa, O, make):
    """50 steps on the device with nothing read in between: the state of the stepwise run, and the same bytes twice"""
    a = _chain(rsa)
    b = _chain(rsa)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes() and a[3].tolist() == b[3].tolist()
    d = F.scene_lattice(make, 3, 3, 5, steps=50)     # (compared with the reference after every step)
    r, tot = d.eng.fwd_read()
    pk, ln = d.eng.fwd_queue_read()
    assert a[0].tobytes() == r.tobytes() and a[1] == tot and a[2].tobytes() == pk.tobytes() and a[3].tolist() == ln.tolist()
    assert tot["arrived"] >= 1 and tot["generated"] > 30


# ---- the source list where a unit walks more than one round --------------------------------------------------------------------

def multi_round_set():
    """-> (n, the nodes of two whole units straddling node 65 536, every third node of the two units after them, and node n - 1) in a
    table of MULTI_ROUND nodes, whose units walk two rounds of 64 nodes"""
    n, chunk = MULTI_ROUND, _chunk(MULTI_ROUND)
    first = 65536 - chunk
    assert chunk == 128 and first % chunk == 0 and (n - 1) // chunk * chunk + 64 < n      # (the last unit's second round is partial)
    return n, list(range(first, first + 2 * chunk)) + list(range(first + 2 * chunk, first + 4 * chunk, 3)) + [n - 1]


def multi_round_caps(count):
    """a cut in the second round of the first unit, in the second round of the second, at the units' end, none, and room to spare"""
    chunk = _chunk(MULTI_ROUND)
    return (64 + 36, chunk + 64 + 10, 2 * chunk, count, count + 44)


def cut_list(nodes, cap):
    """what a source list of `nodes` (ascending) holds under cap: cut at cap, -1 behind the count"""
    return (nodes + [-1] * cap)[:cap]


def test_sources_of_units_of_several_rounds(rsa):
    """a bare table of MULTI_ROUND nodes, no medium work: the unit's running position carries over to its second round and cap cuts
    inside a later round; count is the whole count every time"""
    n, nodes = multi_round_set()
    eng = _bare(rsa, n)
    try:
        eng.fwd_enable()
        eng.fwd_set_next(np.arange(-1, n - 1), [0], 0)        # a line toward node 0
        eng.fwd_inject(nodes, 0)
        for cap in multi_round_caps(len(nodes)):
            got, count = eng.fwd_sources(0, cap)
            assert count == len(nodes) and got.tolist() == cut_list(nodes, cap), cap
    finally:
        eng.close()


# ---- kernel names and launches per call, sampling ------------------------------------------------------------------------------

def launches(eng, prefixes):
    return {k: v[0] for k, v in eng.profile_kernels().items() if k.startswith(prefixes)}


def launches_added(eng, prefix, call):
    """what `call` adds to the sampled launches of the kernels named prefix*"""
    before = launches(eng, prefix)
    call()
    return {k: v - before.get(k, 0) for k, v in launches(eng, prefix).items() if v != before.get(k, 0)}


def lattice_engine(rsa, nd, every_n):
    eng = rsa.Engine(0)
    eng.upload_table(nd)
    eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in F.LATTICE.items()})
    eng.profile_enable(every_n)
    return eng


def test_launches_per_call(rsa, O):
    """a source list is three launches and an advance of a non-empty slot four, each kernel under its name once"""
    nd = F.lattice_nodes()
    eng = lattice_engine(rsa, nd, 1)
    src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
    try:
        eng.fwd_enable()
        eng.fwd_set_next(np.arange(-1, nd.n - 1), [0], 0)
        eng.fwd_inject(list(range(nd.n)), 0)
        added = launches_added(eng, "k_fwd_", lambda: eng.fwd_sources(100, nd.n))
        assert added == {"k_fwd_src_count": 1, "k_fwd_src_scan": 1, "k_fwd_src_write": 1}, added
        eng.tick_run_sources_device(0, F.TICK, src.ptr.value, 27, 100, F.AIR)
        added = launches_added(eng, "k_fwd_", lambda: eng.fwd_advance(0))
        assert added == {"k_fwd_adv_claim": 1, "k_fwd_adv_match": 1, "k_fwd_adv_accept": 1, "k_fwd_adv_apply": 1}, added
        assert eng.fwd_read()[1]["generated"] == nd.n
    finally:
        src.free()
        eng.close()


# what the interleaved calls of the test below launch: their kernels' names begin with one of these, no kernel of a tick's does
FEATURE_KERNELS = ("k_fwd_", "k_flood_", "k_traffic_", "k_hop_", "k_nb_", "k_energy_")


def _seven_ticks(rsa, nd, interleave):
    """7 lone ticks under rm_profile_enable(3), the features on; interleave: a source list of either relay feature, a generated
    traffic row, a hop query and an energy query between the ticks -> {kernel: sampled launches}"""
    eng = lattice_engine(rsa, nd, 3)
    src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
    try:
        eng.fwd_enable()
        eng.fwd_set_next(np.arange(-1, nd.n - 1), [0], 0)
        eng.fwd_inject(list(range(nd.n)), 0)
        eng.flood_enable(imin_us=2)
        eng.flood_seed(list(range(nd.n)), 0)
        eng.traffic_set(np.asarray(F.lattice_table(nd.n, 0), dtype=np.int64))
        eng.profile_enable(3)                                   # (anew: nothing of the set-up above is in the record)
        for k in range(7):
            t = k * F.TICK
            eng.tick_run_sources_device(t, t + F.TICK, src.ptr.value, 27, t + 100, F.AIR)
            if interleave:
                eng.fwd_sources(t + 100, nd.n)
                eng.flood_sources(t + 100, nd.n)
                eng.traffic_generate(5, [t], [t + F.TICK], nd.n)
                eng.hops(H.HEARD_BY, [0])
                eng.channel_energy(t + 500)
        return launches(eng, "k_")
    finally:
        src.free()
        eng.close()


def test_feature_calls_do_not_move_the_ticks_sampling(rsa, O):
    """every third launch sequence is sampled, and a call that is no tick puts the sequence count back: the ticks' kernels are
    sampled as often with feature calls between the ticks as without; the calls themselves are sampled where the next tick is"""
    nd = F.lattice_nodes()
    plain, mixed = _seven_ticks(rsa, nd, False), _seven_ticks(rsa, nd, True)
    ticks_of = lambda m: {k: v for k, v in m.items() if not k.startswith(FEATURE_KERNELS)}
    assert ticks_of(plain) == plain and plain                     # (no feature kernel without a feature call)
    assert ticks_of(mixed) == plain
    for prefix in FEATURE_KERNELS:
        assert any(k.startswith(prefix) for k in mixed), (prefix, sorted(mixed))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _code(rsa, call):
    with pytest.raises(rsa.RadioMediumError) as e:
        call()
    return e.value.code


def test_refusals_leave_the_state_unchanged(rsa, O, make):
    d = F.scene_reroute(make)      # (a state with history)
    eng, n = d.eng, d.nd.n
    d.inject([6, 7, 1], 10 ** 7)
    L, h = eng._L, eng._h
    src = np.array([1, 2, 3], dtype=np.int32)
    par = np.arange(-1, n - 1, dtype=np.int32)
    dv = d.dev(src)
    cnt = C.c_int32(0)
    # INVALID: NULL arguments, negative counts and times, cap < 1, a slot outside the last call's, a bad host index
    calls = [lambda: L.rm_fwd_set_next(h, None, None, 0, 0), lambda: L.rm_fwd_set_next(h, par.ctypes.data, None, 1, 0),
             lambda: L.rm_fwd_set_next(h, par.ctypes.data, src.ctypes.data, -1, 0), lambda: L.rm_fwd_set_next(h, par.ctypes.data, src.ctypes.data, 3, -1),
             lambda: L.rm_fwd_set_next(h, par.ctypes.data, np.array([n], dtype=np.int32).ctypes.data, 1, 0),
             lambda: L.rm_fwd_set_next_device(h, None, None, 0, 0), lambda: L.rm_fwd_set_next_device(h, dv.ptr.value, None, 2, 0),
             lambda: L.rm_fwd_inject(h, None, 3, 0), lambda: L.rm_fwd_inject(h, src.ctypes.data, -1, 0), lambda: L.rm_fwd_inject(h, src.ctypes.data, 3, -5),
             lambda: L.rm_fwd_inject(h, np.array([1, n + 3], dtype=np.int32).ctypes.data, 2, 0), lambda: L.rm_fwd_inject_device(h, None, 3, 0),
             lambda: L.rm_fwd_inject_device(h, dv.ptr.value, -2, 0), lambda: L.rm_fwd_inject_device(h, dv.ptr.value, 3, -1),
             lambda: L.rm_fwd_sources(h, 0, 0, src.ctypes.data, C.byref(cnt)),
             lambda: L.rm_fwd_sources(h, -1, 3, src.ctypes.data, C.byref(cnt)),
             lambda: L.rm_fwd_sources(h, 0, 3, None, C.byref(cnt)),
             lambda: L.rm_fwd_sources_device(h, 0, -1, dv.ptr.value, dv.ptr.value), lambda: L.rm_fwd_sources_device(h, 0, 3, None, dv.ptr.value),
             lambda: L.rm_fwd_advance(h, 1, None, 0), lambda: L.rm_fwd_advance(h, -1, None, 0), lambda: L.rm_fwd_advance(h, 0, src.ctypes.data, -1),
             lambda: L.rm_fwd_advance_device(h, 7, None, 0), lambda: L.rm_fwd_advance_device(h, 0, dv.ptr.value, -1),
             lambda: L.rm_fwd_read(h, None, 3, None, None), lambda: L.rm_fwd_read(h, src.ctypes.data, -1, None, None),
             lambda: L.rm_fwd_read(h, np.array([n], dtype=np.int32).ctypes.data, 1, par.ctypes.data, None),
             lambda: L.rm_fwd_queue_read(h, src.ctypes.data, 3, None, None), lambda: L.rm_fwd_enable(h, None)]
    for k, call in enumerate(calls):
        assert call() == INVALID, k
    bad = eng.fwd_params(queue_slots=3)
    assert _code(rsa, lambda: eng.fwd_enable(bad)) == INVALID and eng.fwd_enabled()
    same_state(eng, d.ref, "after the INVALID refusals")
    assert cnt.value == 0 and src.tolist() == [1, 2, 3]
    # STATE: a receiver partition (a gathered form: test_advance_after_a_gathered_form_is_refused)
    eng.set_partition(0, n // 2)
    assert _code(rsa, lambda: eng.fwd_advance(0)) == STATE
    eng.set_partition(0, n)
    same_state(eng, d.ref, "after the STATE refusal")
    # off: every call but enable / enabled / disable is refused; enable again starts from nothing
    eng.fwd_disable()
    assert not eng.fwd_enabled()
    for call in (lambda: eng.fwd_advance(0), lambda: eng.fwd_read(), lambda: eng.fwd_inject([1], 0), lambda: eng.fwd_sources(0, 4),
                 lambda: eng.fwd_set_next(par, [0], 0), lambda: eng.fwd_reset(), lambda: eng.fwd_device(), lambda: eng.fwd_queue_read()):
        assert _code(rsa, call) == STATE
    eng.fwd_enable(queue_slots=2)
    rows, tot = eng.fwd_read()
    assert (rows["next"] == F.NO_ROUTE).all() and not any(tot.values()) and not rows["queue_len"].any()
    # another node count switches the feature off; the same node count keeps everything
    eng.fwd_set_next(par, [0], 0)
    eng.fwd_inject([1, 2, 2, 2], 5)
    before = eng.fwd_read()
    eng.upload_table(d.nd)
    eng.update_node(1, 3.0, 0.0, 0.0, 0.0, int(d.nd.channel[1]), 1, 1.0, 1.0)
    after = eng.fwd_read()
    assert before[0].tobytes() == after[0].tobytes() and before[1] == after[1] and after[1]["dropped_full"] == 1
    eng.upload_table(F.line_nodes(n + 1))
    assert not eng.fwd_enabled()


def test_advance_after_a_gathered_form_is_refused(rsa, O, make):
    """the last evaluating call was a gathered form (rm_dist_* and rm_group_* leave the same mark): STATE, nothing changes; a lone
    tick after it is advanced again"""
    nd = F.lattice_nodes()
    d = make(nd, "logdist", F.N.PLAIN, queue_slots=4)     # (81 nodes: a sorted receiver table, which the gathered forms need)
    d.set_next(d.tree([0]), [0], 0)
    d.inject(list(range(1, nd.n, 2)), 0)
    lst = [1, 31, 61]
    dv = d.dev(np.asarray(lst, dtype=np.int32))
    d.eng.batch_run_gathered_sources_device([F.TICK], [2 * F.TICK], dv.ptr.value, 1, 3, [F.TICK + 100], F.AIR)
    assert _code(rsa, lambda: d.eng.fwd_advance(0)) == STATE
    assert _code(rsa, lambda: d.eng.fwd_advance_device(0, dv.ptr.value, 3)) == STATE
    same_state(d.eng, d.ref, "after the refusals")
    t = 4 * F.TICK
    d.advance(d.tick(t, t + F.TICK, lst, t + 100, F.AIR))
    assert sum(d.ref.c["attempts"]) == 3


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import radio_sim_amd as rsa
import fwd_ref as F
eng = rsa.Engine(0)
eng.upload_table(F.line_nodes(8))
for call in (lambda: eng.fwd_enable(), lambda: eng.fwd_advance(0), lambda: eng.fwd_inject([1], 0)):
    try:
        call()
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        print("REFUSED", "RM_GRAPH" in str(e))
    else:
        print("ACCEPTED")
print(int(eng.fwd_enabled()))
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
    assert p.stdout.split() == ["REFUSED", "True", "REFUSED", "False", "REFUSED", "False", "0"], p.stdout


def test_enable_without_nodes_is_refused(rsa):
    eng = rsa.Engine(0)
    try:
        assert _code(rsa, lambda: eng.fwd_enable()) == STATE and not eng.fwd_enabled()
        assert _code(rsa, lambda: eng.fwd_get_params()) == STATE
        eng.upload_table(F.line_nodes(3))
        eng.fwd_enable(queue_slots=16)
        assert eng.fwd_get_params().queue_slots == 16 and eng.fwd_queue_read()[0].shape == (3, 16)
    finally:
        eng.close()


def test_advance_without_a_result_and_off_by_default(rsa, O):
    """no evaluated result yet: STATE.  Off by default: a plain run launches no k_fwd_* kernel, and an existing call's results are
    the same with the feature on"""
    nd = F.lattice_nodes()
    outs = []
    for on in (False, True):
        eng = rsa.Engine(0)
        try:
            eng.upload_table(nd)
            eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in F.LATTICE.items()})
            eng.profile_enable(1)
            if on:
                eng.fwd_enable()
                assert _code(rsa, lambda: eng.fwd_advance(0)) == STATE
                eng.fwd_set_next(np.arange(-1, nd.n - 1), [0], 0)
                eng.fwd_inject(list(range(nd.n)), 0)
            src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
            try:
                eng.tick_run_sources_device(0, F.TICK, src.ptr.value, 27, 100, F.AIR)
                r = eng.result_copy(27)
                if on:
                    eng.fwd_advance(0)
                    assert eng.fwd_read()[1]["generated"] == nd.n
            finally:
                src.free()
            outs.append((r.count, r.pkt.tobytes(), r.dst.tobytes(), r.verdict.tobytes(), r.rssi.tobytes(), r.sinr.tobytes(), r.pkt_offset.tobytes()))
            names = [k for k in eng.profile_kernels() if k.startswith("k_fwd_")]
            assert bool(names) == on, names
        finally:
            eng.close()
    assert outs[0] == outs[1]
