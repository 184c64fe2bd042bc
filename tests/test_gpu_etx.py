"""The measured-route query (rm_etx_*, rm_etx.hip) on the GPU.  Expected routes come from tests/etx_ref.py
alone (tests/test_etx_ref.py holds the scenes' conditions for that reference) and, beside it, from rm_etx_from_tables.  Every
comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import etx_ref as E
from util import DeviceArray

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5
TICK, AIR = 1000, 4256
N_SRC, N_TICKS, ROOTS = 40, 100, [33, 36]   # (a hundred ticks: under this interference forty leave most entries below min_heard)
OPTIONAL = E.FIELDS[1:]
DT = {"cost": np.uint64, "parent": np.int32, "slot": np.int32, "link_cost": np.uint32, "children": np.int32}
CASES = E.cases()


def _bare(rsa, n):
    eng = rsa.Engine(0)
    eng.upload_nodes(np.zeros(n), np.arange(n, dtype=np.float64))
    return eng


def _p(rsa, p):
    return rsa.Engine.etx_params(**p)


def _etx_kernels(eng):
    return {k: v[0] for k, v in eng.profile_kernels().items() if k.startswith("k_etx_")}


class Dev:
    """device copies of a scene's tables, freed together"""

    def __init__(self, peer, heard, delivered):
        self.keep = []
        self.K = peer.shape[1]
        self.tables = (self.put(peer), self.put(E.stats(heard, delivered)), self.K)

    def put(self, a):
        self.keep.append(DeviceArray(np.ascontiguousarray(a)))
        return self.keep[-1].ptr.value

    def free(self):
        for d in self.keep:
            d.free()


def _device_query(eng, dev, params, roots, n, cur=None, alias=False, leave_out=(), tables="own"):
    """the device form into buffers filled with a pattern -> (outputs, totals) as the host form returns them; alias: cur lies in
    the parent buffer itself"""
    bufs = {f: DeviceArray(np.full(n, 0x5A5A5A5A, dtype=DT[f])) for f in DT if f not in leave_out}
    extra = []
    try:
        d_roots = dev.put(np.asarray(roots, dtype=np.int32)) if len(roots) else None
        d_cur = None
        if cur is not None and alias:
            bufs["parent"].free()
            bufs["parent"] = DeviceArray(np.ascontiguousarray(cur, dtype=np.int32))
            d_cur = bufs["parent"].ptr.value
        elif cur is not None:
            extra.append(DeviceArray(np.ascontiguousarray(cur, dtype=np.int32)))
            d_cur = extra[0].ptr.value
        ptr = {f: (bufs[f].ptr.value if f in bufs else None) for f in DT}
        tot = eng.etx_routes_device(params, d_roots, len(roots), ptr["cost"], ptr["parent"], ptr["slot"], ptr["link_cost"], ptr["children"],
                                    dev_cur_ptr=d_cur, dev_tables=dev.tables if tables == "own" else tables)
        out = {f: DeviceArray.read(bufs[f].ptr.value, DT[f], n) for f in bufs}
        if cur is not None and not alias:
            np.testing.assert_array_equal(DeviceArray.read(d_cur, np.int32, n), cur)     # (cur is read, never written)
        return out, tot
    finally:
        for d in list(bufs.values()) + extra:
            d.free()


def _host_query_in_place(rsa, eng, prm, host_tables, roots, cur):
    """rm_etx_query with cur == out->parent (a raw call: Engine.etx_routes always makes fresh outputs) -> (outputs, totals)"""
    n = len(cur)
    out = {f: np.full(n, 0x5A5A5A5A, dtype=DT[f]) for f in DT}
    out["parent"][:] = cur
    idx = np.ascontiguousarray(roots, dtype=np.int32)
    tb = rsa.EtxTables(peer=host_tables[0].ctypes.data, stats=host_tables[1].ctypes.data, K=host_tables[0].shape[1], reserved=0)
    st = rsa.EtxOut(**{f: a.ctypes.data for f, a in out.items()})
    tot = rsa.EtxTotals()
    rsa._lib.check(eng._L.rm_etx_query(eng._h, C.byref(prm), C.byref(tb), idx.ctypes.data if len(idx) else None, len(idx), out["parent"].ctypes.data,
                                       C.byref(st), C.byref(tot)))
    return out, rsa.Engine._etx_totals(tot)


def _all_forms(rsa, eng, dev, s, what):
    """host and device forms, both modes, cur NULL / given / in the parent buffer (both forms), the optional outputs NULL in turn"""
    peer, heard, delivered = s["tables"]
    n = peer.shape[0]
    host_tables = (peer, E.stats(heard, delivered))
    roots = s["roots"]
    for mode in E.MODES:
        p = dict(s["prm"], mode=mode)
        prm = _p(rsa, p)
        for cur in (None, s["cur"]) if s["cur"] is not None else (None,):
            w = "%s mode=%d cur=%s" % (what, mode, cur is not None)
            want = E.tree(peer, heard, delivered, p, roots, cur)
            E.same(*rsa.Engine.etx_from_tables(host_tables, prm, roots, cur), want, w + ", rm_etx_from_tables")
            E.same(*eng.etx_routes(prm, roots, tables=host_tables, cur=cur), want, w + ", host")
            E.same(*_device_query(eng, dev, prm, roots, n, cur), want, w + ", device")
            if cur is not None:
                E.same(*_device_query(eng, dev, prm, roots, n, cur, alias=True), want, w + ", device, cur in the parent buffer")
                E.same(*_host_query_in_place(rsa, eng, prm, host_tables, roots, cur), want, w + ", host, cur in the parent array")
        # every optional output NULL in turn, both forms
        want = E.tree(peer, heard, delivered, p, roots, s["cur"])
        for out in OPTIONAL:
            got, tot = _device_query(eng, dev, prm, roots, n, s["cur"], leave_out=(out,))
            assert set(got) == set(E.FIELDS) - {out}
            E.same(got, tot, want, "%s mode=%d device without %s" % (what, mode, out))
            got, tot = eng.etx_routes(prm, roots, tables=host_tables, cur=s["cur"], fields=(out,))
            assert set(got) == {"cost", out}
            E.same(got, tot, want, "%s mode=%d host with %s alone" % (what, mode, out))
        E.same(*_device_query(eng, dev, prm, roots, n, s["cur"], leave_out=OPTIONAL), want, "%s mode=%d device, cost alone" % (what, mode))


# ---- 1. every scene against the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_scene(rsa, name):
    s = dict(CASES)[name]
    n = s["tables"][0].shape[0]
    eng, dev = _bare(rsa, n), Dev(*s["tables"])
    try:
        _all_forms(rsa, eng, dev, s, name)
        rounds, examined = eng.etx_last_work()
        assert rounds >= (1 if len(s["roots"]) else 0)
    finally:
        dev.free()
        eng.close()


def test_chains_take_n_rounds(rsa):
    """(1025, 2) and (257, 1): the front advances one node per round, and one launch per round"""
    for n, K in E.BANDS[2:]:
        t = E.band(n, K)
        eng, dev = _bare(rsa, n), Dev(*t)
        try:
            eng.profile_enable(1)
            prm = _p(rsa, E.prm(**E.BAND_P))
            got, tot = _device_query(eng, dev, prm, [0], n)
            assert tot["reached"] == n
            rounds, examined = eng.etx_last_work()
            assert rounds == n and examined >= n - 1
            assert _etx_kernels(eng)["k_etx_relax<%d>" % K] == n
        finally:
            dev.free()
            eng.close()


def test_wide(rsa):
    """131 143 nodes, K = 8, roots at both ends: 513 workgroups a round, a shallow tree"""
    t = E.wide()
    n = t[0].shape[0]
    eng, dev = _bare(rsa, n), Dev(*t)
    try:
        cur = None
        for mode in E.MODES:
            p = E.prm(mode=mode, **E.BAND_P)
            want = E.tree_np(*t, p, [0, n - 1], cur)
            got, tot = _device_query(eng, dev, _p(rsa, p), [0, n - 1], n, cur, alias=cur is not None)
            E.same(got, tot, want, "wide mode=%d" % mode)
            assert tot["reached"] == n and eng.etx_last_work()[0] < 400
            if cur is not None:
                assert tot["kept"] > 1000 and tot["switched"] > 1000
            for out in OPTIONAL + (OPTIONAL,):
                leave = out if isinstance(out, tuple) else (out,)
                got, tot = _device_query(eng, dev, _p(rsa, p), [0, n - 1], n, cur, leave_out=leave)
                assert set(got) == set(E.FIELDS) - set(leave)
                E.same(got, tot, want, "wide mode=%d device without %s" % (mode, leave))
            cur = want["parent"]       # (the INBOUND tree is BOTH's current tree)
        host_tables, want = (t[0], E.stats(t[1], t[2])), E.tree_np(*t, p, [0, n - 1], cur)
        E.same(*eng.etx_routes(_p(rsa, p), [0, n - 1], tables=host_tables, cur=cur), want, "wide, host")
        E.same(*_host_query_in_place(rsa, eng, _p(rsa, p), host_tables, [0, n - 1], cur), want, "wide, host, cur in the parent array")
    finally:
        dev.free()
        eng.close()


def test_device_roots_outside_the_table(rsa):
    """-1, n_nodes, INT32_MIN and INT32_MAX in a device root list are ignored; the host form refuses them"""
    t = E.band(300, 4)
    eng, dev = _bare(rsa, 300), Dev(*t)
    try:
        p = E.prm(**E.BAND_P)
        roots = E.root_lists(300)["outside"]
        want = E.tree(*t, p, roots)
        assert want["totals"]["roots"] == 3
        E.same(*_device_query(eng, dev, _p(rsa, p), roots, 300), want, "outside")
        E.same(*_device_query(eng, dev, _p(rsa, p), [-1, 300], 300), E.tree(*t, p, []), "no valid root")
        with pytest.raises(rsa.RadioMediumError) as e:
            eng.etx_routes(_p(rsa, p), roots, tables=(t[0], E.stats(t[1], t[2])))
        assert e.value.code == INVALID
    finally:
        dev.free()
        eng.close()


# ---- 2. the context's own tables --------------------------------------------------------------------------------------------------

def _field(rsa, n=400):
    import neighbors_ref as N
    from test_gpu_cca import _engine
    nd = N.rich(n, 14)
    eng = _engine(rsa, nd, dict(N.SHADOW, **N.SINR), 1 << 20)
    eng.set_error_model(rsa.EM_OQPSK_250K)
    eng.seed(7)
    return nd, eng


def _watch_and_run(rsa, eng, n, K, ticks, seed, keep, first_tick=0):
    """neighbors(NB_HEARS, K) -> rm_linkstats_watch_device on the device (first call only), then `ticks` lone ticks of N_SRC sources
    whose frames end inside their tick (a node transmits some ten times in a hundred ticks; a tick's frames interfere with each other)"""
    if first_tick == 0:
        eng.linkstats_enable(K)
        stage = eng.linkstats_stage_device()
        eng.neighbors_device(rsa.NB_HEARS, K, stage)
        eng.linkstats_watch_device(stage)
    rng = np.random.default_rng(seed)
    for k in range(first_tick, first_tick + ticks):
        src = DeviceArray(np.sort(rng.choice(n, N_SRC, replace=False)).astype(np.int32))
        keep.append(src)
        eng.tick_run_sources_device(k * TICK, (k + 1) * TICK, src.ptr.value, N_SRC, k * TICK, 400)


def test_own_tables(rsa, O):
    """a log-distance field with shadowing, interference and the frame error model; tables = NULL is the reference applied to what
    rm_linkstats_peers_get / rm_linkstats_read return; the query changes neither the E14 tables nor the generator nor a later tick"""
    keep = []
    (nd, a), (_, b) = _field(rsa), _field(rsa)
    try:
        b.profile_enable(1)   # every launch of the context that never asks is recorded, from its first tick on
        for e in (a, b):
            _watch_and_run(rsa, e, nd.n, 8, N_TICKS, 3, keep)
        peers, (table, totals) = a.linkstats_peers(), a.linkstats_read()
        assert totals["ticks_counted"] == N_TICKS and (table["heard"] > table["delivered"]).sum() > 50 and (table["delivered"] > 0).sum() > 200
        state = a.rng_state
        a.profile_enable(1)
        for mode in E.MODES:
            for kw in ({}, {"min_heard": 1, "max_link_cost": 1024}):
                p = E.prm(mode=mode, **kw)
                want = E.tree(peers, table["heard"], table["delivered"], p, ROOTS)
                assert want["totals"]["reached"] > (100 if mode == E.INBOUND else 50) and (want["link_cost"] > 128).sum() > 20
                got, tot = a.etx_routes(_p(rsa, p), ROOTS)
                E.same(got, tot, want, "own tables mode=%d %s" % (mode, kw))
                cur = np.roll(want["parent"], 1)
                E.same(*a.etx_routes(_p(rsa, p), ROOTS, cur=cur), E.tree(peers, table["heard"], table["delivered"], p, ROOTS, cur), "own tables, cur")
        asked = _etx_kernels(a)
        assert set(asked) == {"k_etx_cost<8>", "k_etx_init", "k_etx_seed", "k_etx_relax<8>", "k_etx_parent<8>", "k_etx_totals"}
        after = a.linkstats_read()
        assert after[0].tobytes() == table.tobytes() and after[1] == totals and a.rng_state == state == b.rng_state
        np.testing.assert_array_equal(a.linkstats_peers(), peers)
        for e in (a, b):   # a lone tick behind the queries is the tick of the context that never asked
            _watch_and_run(rsa, e, nd.n, 8, 1, 4, keep, first_tick=N_TICKS + 5)
        ra, rb = a.result_copy(N_SRC, cap=1 << 16), b.result_copy(N_SRC, cap=1 << 16)
        assert ra.count == rb.count > 0 and ra.verdict.tobytes() == rb.verdict.tobytes() and ra.dst.tobytes() == rb.dst.tobytes()
        assert a.rng_state == b.rng_state and a.linkstats_read()[0].tobytes() == b.linkstats_read()[0].tobytes()
        # no evaluating call launches a kernel of the query: a's counts did not move over its tick behind the queries, and b, whose
        # hundred and one ticks, neighbour query and watch were all recorded, never launched one
        assert _etx_kernels(a) == asked and len(a.profile_kernels()) > len(asked)
        recorded = b.profile_kernels()
        assert 5 < len(recorded) < 64 and "k_linkstats" in " ".join(recorded) and sum(v[0] for v in recorded.values()) > N_TICKS
        assert not [k for k in recorded if k.startswith("k_etx_")]
    finally:
        for d in keep:
            d.free()
        a.close()
        b.close()


# ---- 3. the chain: counters -> routes -> next hops and a K = 1 watch, nothing through the host -----------------------------------

def test_chain(rsa, O):
    keep = []
    nd, eng = _field(rsa)
    n = nd.n

    def dev(a):
        keep.append(DeviceArray(np.ascontiguousarray(a)))
        return keep[-1].ptr.value

    try:
        _watch_and_run(rsa, eng, n, 8, N_TICKS, 3, keep)
        d_cost, d_par, d_root = dev(np.zeros(n, dtype=np.uint64)), dev(np.full(n, -9, dtype=np.int32)), dev(np.array(ROOTS[:1], dtype=np.int32))
        p0 = E.prm(hysteresis=0)
        tot = eng.etx_routes_device(_p(rsa, p0), d_root, 1, d_cost, d_par)
        peers, (table, _) = eng.linkstats_peers(), eng.linkstats_read()
        first = E.tree(peers, table["heard"], table["delivered"], p0, ROOTS[:1])
        assert tot == first["totals"] and tot["reached"] > 100
        np.testing.assert_array_equal(DeviceArray.read(d_par, np.int32, n), first["parent"])
        # the parents as next hops and as a K = 1 watch
        eng.fwd_enable(queue_slots=4)
        eng.fwd_set_next_device(d_par, d_root, 1, 0)
        rows, _ = eng.fwd_read()
        np.testing.assert_array_equal(np.delete(rows["next"], ROOTS[0]), np.delete(first["parent"], ROOTS[0]))
        # a second window, queried with cur = parent in place, hysteresis 0 and 192
        eng.linkstats_reset()
        _watch_and_run(rsa, eng, n, 8, N_TICKS, 5, keep, first_tick=N_TICKS + 50)
        table2 = eng.linkstats_read()[0]
        assert table2.tobytes() != table.tobytes()
        seen = []
        for h in (0, 192):
            p = E.prm(hysteresis=h)
            want = E.tree(peers, table2["heard"], table2["delivered"], p, ROOTS[:1], first["parent"])
            d_par2 = dev(first["parent"])
            tot = eng.etx_routes_device(_p(rsa, p), d_root, 1, d_cost, d_par2, dev_cur_ptr=d_par2)
            assert tot == want["totals"]
            np.testing.assert_array_equal(DeviceArray.read(d_par2, np.int32, n), want["parent"])
            seen.append((tot["kept"], tot["switched"]))
        assert seen[0][0] > 0 and seen[0][1] > 0 and seen[1][0] >= seen[0][0]
        eng.fwd_set_next_device(d_par2, d_root, 1, 300 * TICK)
        eng.linkstats_enable(1)
        eng.linkstats_watch_device(d_par2)
        np.testing.assert_array_equal(eng.linkstats_peers().reshape(-1), want["parent"])
        # E19 advances a few ticks along the measured routes
        d_src, d_count = dev(np.full(n + 8, -1, dtype=np.int32)), dev(np.zeros(1, dtype=np.int32))
        inject = dev(np.flatnonzero(want["parent"] >= 0)[:60].astype(np.int32))
        eng.fwd_inject_device(inject, 60, 300 * TICK)
        for k in range(300, 308):
            eng.fwd_sources_device(k * TICK + 100, n, d_src, d_count)
            eng.tick_run_sources_device(k * TICK, (k + 1) * TICK, d_src, n, k * TICK + 100, 400)
            eng.fwd_advance_device(0, None, 0)
        t = eng.fwd_read()[1]
        assert t["generated"] == 60 and t["dropped_no_route"] == 0
        assert t["generated"] == t["arrived"] + t["dropped_retries"] + t["dropped_no_route"] + t["dropped_full"] + t["dropped_ttl"] + t["in_flight"]
        assert t["arrived"] + t["dropped_retries"] + t["in_flight"] > 0
    finally:
        for d in keep:
            d.free()
        eng.close()


# ---- 4. launches ------------------------------------------------------------------------------------------------------------------

def test_launches_per_query(rsa):
    t = E.band(300, 4)
    eng, dev = _bare(rsa, 300), Dev(*t)
    try:
        eng.profile_enable(1)
        assert _etx_kernels(eng) == {}
        prm = _p(rsa, E.prm(**E.BAND_P))
        _device_query(eng, dev, prm, [0], 300)
        rounds = eng.etx_last_work()[0]
        assert _etx_kernels(eng) == {"k_etx_cost<4>": 1, "k_etx_init": 1, "k_etx_seed": 1, "k_etx_relax<4>": rounds, "k_etx_parent<4>": 1, "k_etx_totals": 1}
        _device_query(eng, dev, prm, [0], 300, leave_out=OPTIONAL)        # cost alone: no parent pass
        r2 = eng.etx_last_work()[0]
        assert _etx_kernels(eng) == {"k_etx_cost<4>": 2, "k_etx_init": 2, "k_etx_seed": 2, "k_etx_relax<4>": rounds + r2, "k_etx_parent<4>": 1, "k_etx_totals": 2}
        _device_query(eng, dev, prm, [], 300)                              # no roots: no seed, no round
        assert eng.etx_last_work() == (0, 0)
        k = _etx_kernels(eng)
        assert k["k_etx_seed"] == 2 and k["k_etx_relax<4>"] == rounds + r2 and k["k_etx_init"] == 3 and k["k_etx_parent<4>"] == 2
        assert not [name for name in eng.profile_kernels() if not name.startswith("k_etx_")]
    finally:
        dev.free()
        eng.close()


# ---- 5. refusals, each with nothing launched --------------------------------------------------------------------------------------

def _refused(eng, code, fn):
    with pytest.raises(Exception) as e:
        fn()
    assert getattr(e.value, "code", None) == code, e.value
    assert _etx_kernels(eng) == {}, _etx_kernels(eng)


def test_refusals(rsa):
    t = E.band(65, 4)
    n = 65
    eng, dev = _bare(rsa, n), Dev(*t)
    host_tables = (t[0], E.stats(t[1], t[2]))
    cost = DeviceArray(np.zeros(n, dtype=np.uint64))
    root = DeviceArray(np.zeros(4, dtype=np.int32))
    try:
        eng.profile_enable(1)
        L, h = eng._L, eng._h
        st = rsa.EtxOut(cost=cost.ptr.value)
        ok = rsa.Engine.etx_params()
        tb = rsa.EtxTables(peer=dev.tables[0], stats=dev.tables[1], K=4, reserved=0)
        q = lambda *a: rsa._lib.check(L.rm_etx_query_device(*a))
        _refused(eng, INVALID, lambda: q(None, C.byref(ok), C.byref(tb), root.ptr.value, 1, None, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, None, C.byref(tb), root.ptr.value, 1, None, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), C.byref(tb), root.ptr.value, 1, None, None, None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), C.byref(tb), root.ptr.value, 1, None, C.byref(rsa.EtxOut()), None))
        _refused(eng, INVALID, lambda: rsa._lib.check(L.rm_etx_query(h, C.byref(ok), C.byref(tb), root.ptr.value, 1, None, C.byref(rsa.EtxOut()), None)))
        for kw in ({"mode": 2}, {"mode": -1}, {"reserved": 1}, {"reserved2": 1}, {"min_heard": 2 ** 31 + 1}, {"max_link_cost": 127},
                   {"max_link_cost": 65536}, {"hysteresis": 65536}):
            prm = rsa.Engine.etx_params(**kw)
            _refused(eng, INVALID, lambda: eng.etx_routes(prm, [0], tables=host_tables))
            _refused(eng, INVALID, lambda: q(h, C.byref(prm), C.byref(tb), root.ptr.value, 1, None, C.byref(st), None))
        for kw in ({"K": 0}, {"K": 3}, {"K": 16}, {"K": -1}, {"reserved": 1}, {"peer": None}, {"stats": None}, {"peer": dev.tables[0] + 4}):
            bad = rsa.EtxTables(**dict(dict(peer=dev.tables[0], stats=dev.tables[1], K=4, reserved=0), **kw))
            _refused(eng, INVALID, lambda: q(h, C.byref(ok), C.byref(bad), root.ptr.value, 1, None, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), C.byref(tb), root.ptr.value, -1, None, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), C.byref(tb), None, 1, None, C.byref(st), None))
        for roots in ([0, -1], [n], [3, -2 ** 31]):
            _refused(eng, INVALID, lambda: eng.etx_routes(ok, roots, tables=host_tables))
        # tables = NULL needs E14 on and the whole receiver table
        _refused(eng, STATE, lambda: eng.etx_routes(ok, [0]))
        _refused(eng, STATE, lambda: q(h, C.byref(ok), None, root.ptr.value, 1, None, C.byref(st), None))
        eng.linkstats_enable(4)
        eng.set_partition(0, n // 2)
        _refused(eng, STATE, lambda: eng.etx_routes(ok, [0]))
        eng.set_partition(0, n)
        eng.set_partition_spatial(0, 2)
        _refused(eng, STATE, lambda: eng.etx_routes(ok, [0]))
        eng.set_partition_spatial(0, 1)
        eng.tick_begin(0, TICK)
        _refused(eng, STATE, lambda: eng.etx_routes(ok, [0]))
        _refused(eng, STATE, lambda: eng.etx_routes(ok, [0], tables=host_tables))
        eng.enqueue_tx(1, 0, AIR)
        eng.tick_flush(cap=1 << 12)
        # and what is accepted: every medium, an empty watch table, no roots, the parameters' edges
        for kind in (0, 1, 2, 3, 4):
            eng.set_model(kind)
            assert eng.etx_routes(ok, [], tables=host_tables)[1] == {"reached": 0, "roots": 0, "kept": 0, "switched": 0, "lost": 0, "max_cost": 0}
        assert _etx_kernels(eng) != {}
        assert eng.etx_routes(ok, [0])[1] == {"reached": 1, "roots": 1, "kept": 0, "switched": 0, "lost": 0, "max_cost": 0}   # (all slots empty)
        edge = rsa.Engine.etx_params(min_heard=2 ** 31, max_link_cost=65535, hysteresis=65535, mode=1)
        assert eng.etx_routes(edge, [0], tables=host_tables)[1]["reached"] == 1
        assert eng.etx_routes(rsa.Engine.etx_params(max_link_cost=128), [0], tables=host_tables)[1]["reached"] >= 1
    finally:
        cost.free()
        root.free()
        dev.free()
        eng.close()


def test_context_without_nodes(rsa):
    eng = rsa.Engine(0)
    try:
        eng.profile_enable(1)
        peer, st = np.zeros((0, 4), dtype=np.int32), E.stats(np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
        dummy = DeviceArray(np.zeros(16, dtype=np.uint64))
        try:
            assert eng.etx_routes_device(rsa.Engine.etx_params(), None, 0, dummy.ptr.value, dev_tables=(dummy.ptr.value, dummy.ptr.value, 4))["reached"] == 0
        finally:
            dummy.free()
        assert _etx_kernels(eng) == {} and eng.etx_last_work() == (0, 0)
    finally:
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import radio_sim_amd as rsa
import etx_ref as E
eng = rsa.Engine(0)
try:
    eng.upload_nodes(np.zeros(4), np.arange(4.0))
    eng.profile_enable(1)
    t = E.band(4, 2)
    try:
        eng.etx_routes(rsa.Engine.etx_params(), [0], tables=(t[0], E.stats(t[1], t[2])))
    except rsa.RadioMediumError as e:
        assert e.code == -5 and "RM_GRAPH" in str(e), e
        assert not [k for k in eng.profile_kernels() if k.startswith("k_etx_")]
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_query_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)
