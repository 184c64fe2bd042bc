"""The dissemination floods (rm_flood_*, rm_flood.hip) on the GPU.  The scenes are those of
tests/flood_ref.py, played by a driver that sends every call to the engine as well: ticks are the engine's, the reference is advanced
from the result copied out of the engine by rm_result_copy, and after EVERY call the whole node table, the totals, the source lists
(host and device forms in turn: a call rolls the suppression, so one call per step) and rm_flood_tree_device's arrays are compared
with the reference -- exactly.  tests/test_flood_ref.py holds the scenes' conditions for the reference alone."""
import ctypes as C

import numpy as np
import pytest

import flood_ref as F
from test_gpu_fwd import cut_list, launches_added, multi_round_caps, multi_round_set
from test_gpu_traffic import _bare
from util import DeviceArray, KINDS, _PARAM_MAP

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5


def same_state(eng, ref, what, tree=None):
    """the whole table and the totals against the reference; tree = (dev_parent, dev_hop): rm_flood_tree_device's arrays as well"""
    rows, tot = eng.flood_read()
    want = ref.table()
    for f in F.NODE_FIELDS:
        np.testing.assert_array_equal(rows[f].astype(object), np.array(want[f], dtype=object), err_msg="%s: %s" % (what, f))
    assert tot == ref.totals(), (what, tot, ref.totals())
    if tree is not None:
        eng.flood_tree_device(tree[0].ptr.value, tree[1].ptr.value)
        assert DeviceArray.read(tree[0].ptr.value, np.int32, ref.n).tolist() == want["parent"], what + ": tree parent"
        assert DeviceArray.read(tree[1].ptr.value, np.int32, ref.n).tolist() == want["hop"], what + ": tree hop"
    return rows, tot


class GpuDriver(F.Driver):
    """every call to the engine and to the reference; ticks are the engine's"""

    def __init__(self, rsa, nd, kind, params, listen=None, **flood):
        super().__init__(nd, kind, params, listen, **flood)
        self.rsa = rsa
        self.eng = rsa.Engine(0)
        self.eng.upload_table(nd)
        self.eng.set_model(KINDS[kind], **{_PARAM_MAP[k]: v for k, v in params.items()})
        if listen is not None:
            self.eng.listen_set(np.asarray(listen, dtype=np.int64))
        self.eng.flood_enable(**flood)
        self.bufs, self.calls = [], 0
        self.d_src = self.dev(np.full(nd.n + 8, -1, dtype=np.int32))
        self.d_count = self.dev(np.zeros(1, dtype=np.int32))
        self.tree = (self.dev(np.zeros(nd.n, dtype=np.int32)), self.dev(np.zeros(nd.n, dtype=np.int32)))

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
        same_state(self.eng, self.ref, "%s (call %d)" % (what, self.calls), self.tree)

    def seed(self, nodes, time_us):
        if self.calls % 2 and all(j < self.nd.n for j in nodes):      # (the host form refuses an entry >= n_nodes)
            self.eng.flood_seed(nodes, time_us)
        else:
            d = self.dev(np.asarray(nodes, dtype=np.int32))
            self.eng.flood_seed_device(d.ptr.value, len(nodes), time_us)
        super().seed(nodes, time_us)

    def sources(self, time_us, cap):
        assert cap <= self.nd.n + 8
        if self.calls % 2:
            got, n = self.eng.flood_sources(time_us, cap)
            got = got.tolist()
        else:
            self.eng.flood_sources_device(time_us, cap, self.d_src.ptr.value, self.d_count.ptr.value)
            got = DeviceArray.read(self.d_src.ptr.value, np.int32, cap).tolist()
            n = int(DeviceArray.read(self.d_count.ptr.value, np.int32, 1)[0])
        want, count = super().sources(time_us, cap)
        assert (got, n) == (want, count), ("sources", time_us, cap)
        return want, count

    # -- ticks: the engine's, copied out
    def set_capacity(self, cap):
        super().set_capacity(cap)
        self.eng.set_link_capacity(cap)

    def _copied(self, src, copy, start, air, dropped):
        """copy(): the engine's result; a slot over the link capacity has none to copy (rm_result_copy refuses) and is lost"""
        if dropped:
            return F.records_result(self.nd.n, src, start, air, [0] * (len(src) + 1), [], [], [], lost=True)
        r = copy()
        return self.watch(F.records_result(self.nd.n, src, start, air, r.pkt_offset, r.dst, r.verdict, r.rssi))

    def tick(self, t_begin, t_end, src, start, air):
        d = self.dev(np.asarray(src, dtype=np.int32))
        self.eng.tick_run_sources_device(t_begin, t_end, d.ptr.value, len(src), start, air)
        return self._copied(src, lambda: self.eng.result_copy(len(src)), start, air, self.eng.result_count()[1])

    def tick_cca(self, t_begin, t_end, src, start, air, cca_time, threshold):
        flags, _ = self.eng.tick_run_sources_cca(t_begin, t_end, src, start, air, cca_time, threshold)
        kept = np.where(flags != 0, -1, np.asarray(src, dtype=np.int32))
        return self._copied(kept, lambda: self.eng.result_copy(len(src)), start, air, self.eng.result_count()[1])

    def batch(self, t_begin, t_end, lists, starts, air):
        ds = [self.dev(np.asarray(l, dtype=np.int32)) for l in lists]
        self.eng.batch_run_sources_device(t_begin, t_end, [d.ptr.value for d in ds], [len(l) for l in lists], starts, [air] * len(lists))
        return [self._copied(l, lambda: self.eng.batch_result_copy(b, len(l)), starts[b], air, self.eng.batch_result_count(b)[1])
                for b, l in enumerate(lists)]

    def advance(self, res, cand=None, slot=0):
        if cand is not None and self.calls % 2:
            d = self.dev(np.asarray(cand, dtype=np.int32))
            self.eng.flood_advance_device(slot, d.ptr.value, len(cand))
        else:
            self.eng.flood_advance(slot, cand)
        super().advance(res, cand, slot)

    def reset(self):
        self.eng.flood_reset()
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
    d = F.scene_line(make, n)
    rows, tot = d.eng.flood_read()
    assert rows["hop"].tolist() == list(range(n)) and (np.diff(rows["first_us"]) > 0).all() and tot["covered"] == n


@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("k", [1, 0])
def test_clique(O, make, n, k):
    d = F.scene_clique(make, n, k)
    _, tot = d.eng.flood_read()
    assert d.covered_after_first == n
    if k:
        assert tot["suppressed"] > 0 and tot["sent"] * 8 < n
    else:
        assert tot["suppressed"] == 0 and tot["sent"] == 3 * n


def test_lattice(O, make):
    """33 x 33 on the SINR medium with duty-cycled receivers: first receptions decided by the tie-break, collided and missed copies"""
    d = F.scene_lattice(make)
    assert d.log["ties"] >= 1 and d.log["collided"] >= 1 and d.log["steps"] == 60
    assert int(d.eng.listen_missed().sum()) >= 1


def test_foreign(O, make):
    d = F.scene_foreign(make)
    rows, _ = d.eng.flood_read()
    assert d.log["foreign_delivered"] >= 1 and d.log["foreign_collided"] >= 1
    assert not rows["heard"][7:].any() and (rows["first_us"][6:] == -1).all()


@pytest.mark.parametrize("cand", [True, False])
def test_gated(O, make, cand):
    d = F.scene_gated(make, cand)
    rows, tot = d.eng.flood_read()
    assert d.log["deferred_lists"] >= 1 and (tot["deferred"] >= 1) == cand
    if cand:
        assert ((rows["deferred"] > 0) & (rows["sent"] > 0)).any()


@pytest.mark.parametrize("n", [1025, 4097])
def test_big(O, make, n):
    d = F.scene_big(make, n)
    assert d.log["truncated"] >= 2 and d.eng.flood_read()[1]["suppressed"] > 100


def test_batch(O, make):
    """8 ticks in one rm_batch_run_sources_device, an advance per slot: the state of 8 lone ticks with an advance each"""
    a, b = F.scene_batch(make, True), F.scene_batch(make, False)
    ra, ta = a.eng.flood_read()
    rb, tb = b.eng.flood_read()
    assert ra.tobytes() == rb.tobytes() and ta == tb and ta["stray"] >= 2


def test_limits(O, make):
    d = F.scene_max_hops(make)
    assert (d.eng.flood_read()[0]["first_us"][3:] == -1).all()
    d = F.scene_one_interval(make)
    rows, _ = d.eng.flood_read()
    assert (rows["fire_us"] == -1).all() and (rows["sent"] + rows["suppressed"] == 1).all()
    d = F.scene_capacity(make)
    assert d.unchanged and d.eng.flood_read()[1]["skipped_slots"] == 1


def _chain(rsa, steps=40):
    """seed -> (sources -> tick with n = cap -> advance) x steps on the device, nothing read in between -> the final state's bytes"""
    nd = F.lattice_nodes()
    n = nd.n
    d = GpuDriver(rsa, nd, "logdist", F.LATTICE, listen=F.lattice_listen(n), **dict(F.LATTICE_FLOOD, imin_us=2 * F.TICK))
    try:
        eng = d.eng
        eng.flood_seed([40], 0)
        for k in range(steps):
            t = k * F.TICK
            eng.flood_sources_device(t + 100, n, d.d_src.ptr.value, d.d_count.ptr.value)
            eng.tick_run_sources_device(t, t + F.TICK, d.d_src.ptr.value, n, t + 100, F.AIR)
            eng.flood_advance_device(0, None, 0)
        return eng.flood_read()
    finally:
        d.close()


def test_chain(rsa, O, make):
    """40 steps on the device with nothing read in between, twice: the same bytes, and the state of the stepwise run"""
    a = _chain(rsa)
    b = _chain(rsa)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    nd = F.lattice_nodes()
    d = make(nd, "logdist", F.LATTICE, listen=F.lattice_listen(nd.n), **dict(F.LATTICE_FLOOD, imin_us=2 * F.TICK))
    d.seed([40], 0)
    F.run_steps(d, 40, nd.n, skip=False)       # (compared with the reference after every call)
    r, tot = d.eng.flood_read()
    assert a[0].tobytes() == r.tobytes() and a[1] == tot and tot["covered"] > 40 and tot["suppressed"] > 0


def test_to_fwd(O, make):
    """the measured tree as it lies in device memory is the forwarding queues' next-hop table, the seed its root: a packet injected
    at the far end arrives with hops = the node's hop in the flood"""
    n = 12
    d = make(F.line_nodes(n), "udgm", F.UDGM, **F.LINE)
    d.seed([0], 0)
    F.run_steps(d, 40 * n, n, stop=lambda d: d.ref.totals()["covered"] == n)
    eng = d.eng
    roots = d.dev(np.array([0], dtype=np.int32))
    eng.flood_tree_device(d.tree[0].ptr.value, None)
    eng.fwd_enable(queue_slots=4, max_retries=15, min_be=0, max_be=0, backoff_unit_us=0)
    eng.fwd_set_next_device(d.tree[0].ptr.value, roots.ptr.value, 1, 0)
    eng.fwd_inject([n - 1], 10 ** 7)
    for k in range(n):
        t = 10 ** 7 + k * F.TICK
        eng.fwd_sources_device(t + 100, n, d.d_src.ptr.value, d.d_count.ptr.value)
        eng.tick_run_sources_device(t, t + F.TICK, d.d_src.ptr.value, n, t + 100, F.AIR)
        eng.fwd_advance_device(0, None, 0)
    rows, tot = eng.fwd_read()
    assert tot["arrived"] == 1 and tot["in_flight"] == 0 and int(rows["hops_sum"][n - 1]) == n - 1
    assert rows["next"].tolist() == [-2] + list(range(n - 1))


# ---- the source list where a unit walks more than one round; kernel names and launches per call ------------------------------------

def test_sources_of_units_of_several_rounds(rsa):
    """a bare table of MULTI_ROUND nodes, no medium work, redundancy 0 (no advance has run: nothing is suppressed): the nodes of the
    seeded set whose first fire time -- rm_flood_fire, the host rule -- has come, under caps that cut inside a later round of a unit.
    A source list does not move an unsuppressed node on: the same call again gives the same list"""
    n, nodes = multi_round_set()
    params = rsa.Engine.flood_params(redundancy=0)
    fire = {j: rsa.Engine.flood_fire(params, j, 0, 0)[1] for j in nodes}
    t_mid, t_all = sorted(fire.values())[len(nodes) // 2], max(fire.values()) + 1
    eng = _bare(rsa, n)
    try:
        eng.flood_enable(params)
        eng.flood_seed(nodes, 0)
        for t in (t_mid, t_all):
            due = [j for j in nodes if fire[j] <= t]
            assert (0 < len(due) < len(nodes)) if t == t_mid else due == nodes
            for cap in multi_round_caps(len(nodes)):
                for again in (False, True):
                    got, count = eng.flood_sources(t, cap)
                    assert count == len(due) and got.tolist() == cut_list(due, cap), (t, cap, again)
        assert eng.flood_read()[1]["suppressed"] == 0
    finally:
        eng.close()


def test_launches_per_call(rsa, O):
    """a source list is three launches and an advance four, each kernel under its name once"""
    nd = F.lattice_nodes()
    eng = rsa.Engine(0)
    src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
    try:
        eng.upload_table(nd)
        eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in F.LATTICE.items()})
        eng.profile_enable(1)
        eng.flood_enable(imin_us=2)
        eng.flood_seed(list(range(nd.n)), 0)
        added = launches_added(eng, "k_flood_", lambda: eng.flood_sources(100, nd.n))
        assert added == {"k_flood_src_count": 1, "k_flood_src_scan": 1, "k_flood_src_write": 1}, added
        eng.tick_run_sources_device(0, F.TICK, src.ptr.value, 27, 100, F.AIR)
        added = launches_added(eng, "k_flood_", lambda: eng.flood_advance(0))
        assert added == {"k_flood_adv_claim": 1, "k_flood_rx_hear": 1, "k_flood_rx_pick": 1, "k_flood_settle": 1}, added
        assert eng.flood_read()[1]["sent"] == 27
    finally:
        src.free()
        eng.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _code(rsa, call):
    with pytest.raises(rsa.RadioMediumError) as e:
        call()
    return e.value.code


def test_refusals_leave_the_state_unchanged(rsa, O, make):
    d = F.scene_max_hops(make)      # (a state with history, and an evaluated result)
    eng, n = d.eng, d.nd.n
    L, h = eng._L, eng._h
    src = np.array([1, 2, 3], dtype=np.int32)
    big = np.array([1, n + 3], dtype=np.int32)
    out = np.zeros(n, dtype=eng.flood_read()[0].dtype)
    dv = d.dev(src)
    cnt = C.c_int32(0)
    # INVALID: NULL arguments, negative counts and times, cap < 1, a slot outside the last call's, a host entry >= n_nodes
    calls = [lambda: L.rm_flood_seed(h, None, 3, 0), lambda: L.rm_flood_seed(h, src.ctypes.data, -1, 0), lambda: L.rm_flood_seed(h, src.ctypes.data, 3, -5),
             lambda: L.rm_flood_seed(h, big.ctypes.data, 2, 0), lambda: L.rm_flood_seed_device(h, None, 3, 0),
             lambda: L.rm_flood_seed_device(h, dv.ptr.value, -2, 0), lambda: L.rm_flood_seed_device(h, dv.ptr.value, 3, -1),
             lambda: L.rm_flood_sources(h, 0, 0, src.ctypes.data, C.byref(cnt)), lambda: L.rm_flood_sources(h, -1, 3, src.ctypes.data, C.byref(cnt)),
             lambda: L.rm_flood_sources(h, 0, 3, None, C.byref(cnt)), lambda: L.rm_flood_sources(h, 0, 3, src.ctypes.data, None),
             lambda: L.rm_flood_sources_device(h, 0, -1, dv.ptr.value, dv.ptr.value), lambda: L.rm_flood_sources_device(h, 0, 3, None, dv.ptr.value),
             lambda: L.rm_flood_sources_device(h, 0, 3, dv.ptr.value, None),
             lambda: L.rm_flood_advance(h, 1, None, 0), lambda: L.rm_flood_advance(h, -1, None, 0), lambda: L.rm_flood_advance(h, 0, src.ctypes.data, -1),
             lambda: L.rm_flood_advance(h, 0, big.ctypes.data, 2),
             lambda: L.rm_flood_advance_device(h, 7, None, 0), lambda: L.rm_flood_advance_device(h, 0, dv.ptr.value, -1),
             lambda: L.rm_flood_read(h, None, 3, None, None), lambda: L.rm_flood_read(h, src.ctypes.data, -1, None, None),
             lambda: L.rm_flood_read(h, np.array([n], dtype=np.int32).ctypes.data, 1, out.ctypes.data, None),
             lambda: L.rm_flood_tree_device(h, None, dv.ptr.value), lambda: L.rm_flood_enable(h, None), lambda: L.rm_flood_get_params(h, None)]
    for k, call in enumerate(calls):
        assert call() == INVALID, k
    for kw in (dict(imin_us=1), dict(doublings=17), dict(max_intervals=0), dict(redundancy=256), dict(max_hops=0)):
        bad = eng.flood_params(**kw)
        assert _code(rsa, lambda: eng.flood_enable(bad)) == INVALID and eng.flood_enabled()
    same_state(eng, d.ref, "after the INVALID refusals", d.tree)
    assert cnt.value == 0 and src.tolist() == [1, 2, 3]
    # STATE: a receiver partition
    eng.set_partition(0, n // 2)
    assert _code(rsa, lambda: eng.flood_advance(0)) == STATE
    eng.set_partition(0, n)
    same_state(eng, d.ref, "after the STATE refusal", d.tree)
    # the same node count keeps everything
    eng.upload_table(d.nd)
    eng.update_node(1, 40.0, 0.0, 0.0, 0.0, int(d.nd.channel[1]), 1, 1.0, 1.0)
    same_state(eng, d.ref, "after an upload of the same node count", d.tree)
    # reset: nobody has the data, the parameters stay
    d.reset()
    assert eng.flood_get_params().max_hops == 2
    # off: every call but enable / enabled / disable is refused; enable again starts from nothing
    eng.flood_seed([0], 5)
    eng.flood_disable()
    assert not eng.flood_enabled()
    for call in (lambda: eng.flood_advance(0), lambda: eng.flood_read(), lambda: eng.flood_seed([1], 0), lambda: eng.flood_sources(0, 4),
                 lambda: eng.flood_reset(), lambda: eng.flood_device(), lambda: eng.flood_get_params(),
                 lambda: eng.flood_tree_device(d.tree[0].ptr.value), lambda: eng.flood_seed_device(dv.ptr.value, 3, 0),
                 lambda: eng.flood_sources_device(0, 3, dv.ptr.value, dv.ptr.value), lambda: eng.flood_advance_device(0, None, 0)):
        assert _code(rsa, call) == STATE
    eng.flood_enable(redundancy=5)
    rows, tot = eng.flood_read()
    assert (rows["first_us"] == -1).all() and not any(tot.values()) and eng.flood_get_params().redundancy == 5
    assert all(p for p in eng.flood_device())
    # another node count switches the feature off
    eng.upload_table(F.line_nodes(n + 1))
    assert not eng.flood_enabled()


def test_advance_after_a_gathered_form_is_refused(rsa, O, make):
    """the last evaluating call was a gathered form (rm_dist_* and rm_group_* leave the same mark): STATE, nothing changes; a lone
    tick after it is advanced again"""
    nd = F.lattice_nodes()
    d = make(nd, "logdist", F.N.PLAIN, **dict(F.LATTICE_FLOOD, imin_us=2))     # (81 nodes: a sorted receiver table, which the gathered forms need)
    d.seed([1, 31, 61], 0)
    lst = [1, 31, 61]
    dv = d.dev(np.asarray(lst, dtype=np.int32))
    d.eng.batch_run_gathered_sources_device([F.TICK], [2 * F.TICK], dv.ptr.value, 1, 3, [F.TICK + 100], F.AIR)
    assert _code(rsa, lambda: d.eng.flood_advance(0)) == STATE
    assert _code(rsa, lambda: d.eng.flood_advance_device(0, dv.ptr.value, 3)) == STATE
    same_state(d.eng, d.ref, "after the refusals", d.tree)
    t = 4 * F.TICK
    d.advance(d.tick(t, t + F.TICK, lst, t + 100, F.AIR))
    assert sum(d.ref.cnt["sent"]) == 3 and d.ref.totals()["covered"] > 3


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import radio_sim_amd as rsa
import flood_ref as F
eng = rsa.Engine(0)
eng.upload_table(F.line_nodes(8))
for call in (lambda: eng.flood_enable(), lambda: eng.flood_advance(0), lambda: eng.flood_seed([1], 0)):
    try:
        call()
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        print("REFUSED", "RM_GRAPH" in str(e))
    else:
        print("ACCEPTED")
print(int(eng.flood_enabled()))
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
        assert _code(rsa, lambda: eng.flood_enable()) == STATE and not eng.flood_enabled()
        assert _code(rsa, lambda: eng.flood_get_params()) == STATE
        eng.upload_table(F.line_nodes(3))
        eng.flood_enable(max_intervals=64)
        assert eng.flood_get_params().max_intervals == 64 and eng.flood_read()[0].shape == (3,)
    finally:
        eng.close()


def test_advance_without_a_result_and_off_by_default(rsa, O):
    """no evaluated result yet: STATE.  Off by default: a plain run launches no k_flood_* kernel, and an existing call's results are
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
                eng.flood_enable(imin_us=2)
                assert _code(rsa, lambda: eng.flood_advance(0)) == STATE
                eng.flood_seed(list(range(nd.n)), 0)
            src = DeviceArray(np.arange(0, nd.n, 3, dtype=np.int32))
            try:
                eng.tick_run_sources_device(0, F.TICK, src.ptr.value, 27, 100, F.AIR)
                r = eng.result_copy(27)
                if on:
                    eng.flood_advance(0)
                    assert eng.flood_read()[1]["sent"] == 27
            finally:
                src.free()
            outs.append((r.count, r.pkt.tobytes(), r.dst.tobytes(), r.verdict.tobytes(), r.rssi.tobytes(), r.sinr.tobytes(), r.pkt_offset.tobytes()))
            names = [k for k in eng.profile_kernels() if k.startswith("k_flood_")]
            assert bool(names) == on, names
        finally:
            eng.close()
    assert outs[0] == outs[1]
