"""The hop query (rm_hops_*, rm_hops.hip) on the GPU.  Expected trees come from the oracle's potential
links through tests/hops_ref.py alone (tests/test_hops_ref.py holds the scenes' conditions for that reference).  Every comparison
is exact: equal integers, equal rssi bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hops_ref as H
import linkstats_ref as LK
import neighbors_ref as N
import unicast_ref as U
from test_gpu_cca import _bits, _engine
from util import DeviceArray

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5
TICK, AIR = 1000, 4256
SENS = -95.0   # the oracle's default sensitivity
OPTIONAL = ("parent", "rssi", "children")


def _hop_kernels(eng):
    return {k for k in eng.profile_kernels() if k.startswith("k_hop_") or k.startswith("k_nb_")}


def _paths(eng):
    """which walking kernels ran: {"boxes", "scan"}"""
    names = [k for k in _hop_kernels(eng) if k.startswith("k_hop_expand") or k.startswith("k_hop_parent")]
    return {"scan" if k.replace(" ", "").endswith("true>") else "boxes" for k in names}


def _device_query(eng, direction, roots, n, min_rssi=-H.INF, leave_out=()):
    """the device form into buffers filled with a pattern -> (outputs, totals) as the host form returns them"""
    dt = dict(H_FIELDS)
    bufs = {f: DeviceArray(np.full(n, 0x5A5A5A5A if f != "rssi" else 7.0, dtype=dt[f])) for f in dt if f not in leave_out}
    dr = DeviceArray(np.ascontiguousarray(roots, dtype=np.int32)) if len(roots) else None
    try:
        ptr = {f: (bufs[f].ptr.value if f in bufs else None) for f in dt}
        tot = eng.hops_device(direction, dr.ptr.value if dr else None, len(roots), ptr["hop"], ptr["parent"], ptr["rssi"], ptr["children"], min_rssi)
        return {f: DeviceArray.read(bufs[f].ptr.value, dt[f], n) for f in bufs}, tot
    finally:
        for d in list(bufs.values()) + [dr]:
            if d is not None:
                d.free()


H_FIELDS = (("hop", np.int32), ("parent", np.int32), ("rssi", np.float64), ("children", np.int32))


def _link_thresholds(nd, found):
    """some link's own rssi at which the link counts and the tree needs it: (r, the next double above r); the reference's trees at
    the two differ"""
    w = H.tree(nd.n, found, [0])
    for j in np.flatnonzero(w["hop"] >= 1).tolist():
        r = float(w["rssi"][j:j + 1].view(np.float64)[0])
        up = float(np.nextafter(r, H.INF))
        a, b = H.tree(nd.n, found, [0], r), H.tree(nd.n, found, [0], up)
        if a["hop"][j] >= 1 and (a["hop"] != b["hop"]).any():
            return r, up
    raise AssertionError("no link of the tree is needed at its own rssi")


# ---- 1. against the reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(N.SCENES))
def test_trees_against_the_reference(rsa, O, name):
    """both directions, the tests' root sets and thresholds, host and device forms, every optional output NULL in turn.  Tables of
    up to 64 nodes are not sorted (the whole-table scan); the larger ones walk the boxes."""
    nd, params, found = H.scene(name)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in H.DIRS:
            mins = [-H.INF, -85.0, SENS, H.INF]
            if name in N.RICH:
                mins += list(_link_thresholds(nd, found[d]))
            for label, roots in H.root_sets(nd, name).items():
                for mr in mins if label in ("0", "0,S", "all") else mins[:2]:
                    what = "%s dir=%d roots=%s min=%r" % (name, d, label, mr)
                    want = H.tree(nd.n, found[d], roots, mr)
                    H.same(*eng.hops(d, roots, mr), want, what + ", host")
                    if mr in (-H.INF, -85.0):
                        H.same(*_device_query(eng, d, roots, nd.n, mr), want, what + ", device")
            want = H.tree(nd.n, found[d], [0])
            for out in OPTIONAL:
                got, tot = _device_query(eng, d, [0], nd.n, leave_out=(out,))
                assert set(got) == {"hop"} | set(OPTIONAL) - {out}
                H.same(got, tot, want, "%s dir=%d device without %s" % (name, d, out))
                got, tot = eng.hops(d, [0], fields=(out,))
                assert set(got) == {"hop", out}
                H.same(got, tot, want, "%s dir=%d host with %s alone" % (name, d, out))
            H.same(*_device_query(eng, d, [0], nd.n, leave_out=OPTIONAL), want, "%s dir=%d device, hop alone" % (name, d))
        assert _paths(eng) == ({"scan"} if nd.n <= 64 else {"boxes"}), _hop_kernels(eng)
    finally:
        eng.close()


# ---- 2. lines: one node per level ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, path", [("line40", "scan"), ("line70", "boxes")])
def test_lines(rsa, O, name, path):
    nd, params, found = H.scene(name)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in H.DIRS:
            for roots in ([0], [nd.n - 1], [nd.n // 2], [0, nd.n - 1]):
                want = H.tree(nd.n, found[d], roots)
                got, tot = eng.hops(d, roots)
                H.same(got, tot, want, "%s dir=%d roots=%s" % (name, d, roots))
            got, tot = eng.hops(d, [0])
            assert tot == {"reached": nd.n, "max_hop": nd.n - 1, "roots": 1} and got["parent"].tolist() == list(range(-1, nd.n - 1))
        assert _paths(eng) == {path}, _hop_kernels(eng)
    finally:
        eng.close()


# ---- 3. frontiers that span many workgroups -----------------------------------------------------------------------------------

def test_n3000(rsa, O):
    """rich(3000, 5): three boxes of 1024 receivers, levels of more than 256 nodes (64 workgroups of frontier waves and more)"""
    nd, params, found = H.scene("n3000_shadow")
    sp = N.special(nd)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in H.DIRS:
            for roots, mr in (([0], -H.INF), ([0], -85.0), ([sp["A"], sp["B"], 17, 17], -H.INF), (list(range(nd.n)), -H.INF)):
                want = H.tree(nd.n, found[d], roots, mr)
                H.same(*eng.hops(d, roots, mr), want, "n3000 dir=%d roots=%s.. min=%r" % (d, roots[:4], mr))
            want = H.tree(nd.n, found[d], [0])
            assert np.bincount(want["hop"][want["hop"] >= 0]).max() > 256
            H.same(*_device_query(eng, d, [0], nd.n), want, "n3000 dir=%d device" % d)
        assert _paths(eng) == {"boxes"}
    finally:
        eng.close()


# ---- 4. 65 537 nodes: the query held to E16 on the same context ---------------------------------------------------------------

def test_large_table_against_the_neighbour_query(rsa, O):
    """the full graph of 65 537 nodes is too large for the oracle; E16's tests hold E16 to the oracle at this size, and this holds
    the query to E16: for every node whose E16 degree is at most 16 the row is the node's whole link set"""
    nd, _ = N.large(65537)
    sp = N.special(nd)
    eng = _engine(rsa, nd, N.SHADOW)
    try:
        for d in H.DIRS:
            nb = eng.neighbors(d, 16)
            got, tot = eng.hops(d, [0, sp["S"]])
            hop, parent = got["hop"].astype(np.int64), got["parent"].astype(np.int64)
            assert tot["roots"] == 2 and tot["reached"] == (hop >= 0).sum() and tot["max_hop"] == hop.max()
            assert hop[0] == 0 and hop[sp["S"]] == 0 and hop[sp["A"]] == 1 and hop[sp["LONE"]] == -1
            whole = nb["degree"] <= 16
            peer = nb["peer"].astype(np.int64)
            valid = peer >= 0
            rh = np.where(valid, hop[np.where(valid, peer, 0)], -1)          # the row entries' hops, -1: none or unreached
            up = (hop - 1)[:, None]
            reached = whole & (hop >= 1)
            assert reached.sum() > 1000 and hop.max() > 10   # (not vacuous: a tree of many levels over more than one round of boxes)
            assert not (reached[:, None] & (rh >= 0) & (rh < up)).any()       # no row entry is closer than one level up
            is_up = valid & (rh == up)
            assert is_up[reached].any(axis=1).all()
            first = np.argmax(is_up, axis=1)
            rows = np.flatnonzero(reached)
            np.testing.assert_array_equal(parent[rows], peer[rows, first[rows]])
            np.testing.assert_array_equal(_bits(got["rssi"])[rows], _bits(nb["rssi"])[rows, first[rows]])
            assert (hop[parent[rows]] == hop[rows] - 1).all()
            unreached = whole & (hop == -1)
            assert unreached.sum() > 0 and not (rh[unreached] >= 0).any()
            assert (parent[hop < 1] == -1).all() and (_bits(got["rssi"])[hop < 1] == N.NAN_BITS).all()
            np.testing.assert_array_equal(got["children"], np.bincount(parent[parent >= 0], minlength=nd.n))
    finally:
        eng.close()


# ---- 5. every state of the table ----------------------------------------------------------------------------------------------

def _update(eng, nd, j, **kw):
    """rm_node_update of node j, mirrored in the reference's table"""
    for k, v in kw.items():
        getattr(nd, k)[j] = v
    eng.update_node(j, nd.x[j], nd.y[j], nd.z[j], nd.txpower[j], int(nd.channel[j]), int(nd.enabled[j]), nd.rxprob[j], nd.txprob[j])


def _check_all(eng, nd, params, what, sp):
    for d in H.DIRS:
        found = N.links(nd, params, d)
        for roots, mr in (([0], -H.INF), ([sp["S"], 5], -H.INF), ([0], -85.0)):
            H.same(*eng.hops(d, roots, mr), H.tree(nd.n, found, roots, mr), "%s dir=%d roots=%s min=%r" % (what, d, roots, mr))


def test_after_node_changes(rsa, O):
    """a node moved out of its group's box (rm_node_update, rm_nodes_move); one far node's txpower raised until other nodes hear it;
    a radio switched off and on; another sensitivity; a node moved outside the fp32 frame (the whole-table scan answers)"""
    nd0, params, _ = N.scene("n300_shadow")
    nd, sp = N._copy(nd0), N.special(nd0)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        _check_all(eng, nd, params, "before", sp)
        _update(eng, nd, 3, x=nd.x[sp["S"]] + 2.0, y=nd.y[sp["S"]] + 1.0)      # from the field to the crafted nodes
        _check_all(eng, nd, params, "rm_node_update: moved far", sp)
        nd.x[[10, 11]], nd.y[[10, 11]] = [nd.x[sp["LONE"]] + 10.0, -300.0], [nd.y[sp["LONE"]], -300.0]
        eng.move_nodes(np.array([10, 11], dtype=np.int32), nd.x[[10, 11]], nd.y[[10, 11]])
        _check_all(eng, nd, params, "rm_nodes_move", sp)
        before = H.tree(nd.n, N.links(nd, params, N.HEARS), [sp["LONE"]])["totals"]["reached"]
        _update(eng, nd, sp["LONE"], txpower=75.0)                             # 5 km and more away: now heard by the crafted nodes
        assert H.tree(nd.n, N.links(nd, params, N.HEARS), [sp["LONE"]])["totals"]["reached"] > before + 5
        for d in H.DIRS:
            H.same(*eng.hops(d, [sp["LONE"]]), H.tree(nd.n, N.links(nd, params, d), [sp["LONE"]]), "the loud lone root dir=%d" % d)
        _check_all(eng, nd, params, "txpower raised", sp)
        _update(eng, nd, sp["A"], enabled=0)
        _update(eng, nd, sp["OFF"], enabled=1)
        _update(eng, nd, 0, enabled=0)                                         # (a root is a root whatever its radio state)
        _check_all(eng, nd, params, "radios switched", sp)
        params2 = dict(params, ld_sensitivity_dbm=-88.5)
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in params2.items()})
        _check_all(eng, nd, params2, "another sensitivity", sp)
        assert _paths(eng) == {"boxes"}
        _update(eng, nd, 20, x=4.0e7, y=-3.0e7)
        _check_all(eng, nd, params2, "outside the fp32 frame", sp)
        assert _paths(eng) == {"boxes", "scan"}
    finally:
        eng.close()


def test_both_kernel_paths(rsa, O):
    """the same scene through the boxes and through the whole-table scan (a far node makes the fp32 frame too coarse for the boxes;
    it hears nobody and nobody hears it): equal bits, and rm_profile_kernels tells which ran"""
    nd0, params, found = N.scene("n300_shadow")
    nd = N._copy(nd0)
    sp = N.special(nd)
    out = {}
    for path in ("boxes", "scan"):
        eng = _engine(rsa, nd, params)
        try:
            eng.profile_enable(1)
            if path == "scan":
                _update(eng, nd, sp["LONE"], x=5.0e7, y=5.0e7)
            out[path] = [eng.hops(d, [0, sp["S"]], mr) for d in H.DIRS for mr in (-H.INF, -85.0)]
            assert _paths(eng) == {path}, _hop_kernels(eng)
            assert "k_nb_prep" in _hop_kernels(eng) and "k_hop_seed" in _hop_kernels(eng)
        finally:
            eng.close()
    k = 0
    for d in H.DIRS:
        for mr in (-H.INF, -85.0):
            (a, ta), (b, tb) = out["boxes"][k], out["scan"][k]
            H.same(a, ta, H.tree(nd0.n, found[d], [0, sp["S"]], mr), "boxes dir=%d min=%r" % (d, mr))
            assert ta == tb
            for f in ("hop", "parent", "children"):
                np.testing.assert_array_equal(a[f], b[f])
            np.testing.assert_array_equal(_bits(a["rssi"]), _bits(b["rssi"]))
            k += 1


# ---- 6. flood equivalence -----------------------------------------------------------------------------------------------------

def test_levels_are_a_flood_of_lone_ticks(rsa, O):
    """every radio on, HEARS, every potential link: level L + 1 is the set of receivers of one lone tick whose sources are level
    L's nodes, minus the nodes labelled before"""
    nd0, params, _ = N.scene("n300_shadow")
    nd = N._copy(nd0)
    nd.enabled[:] = 1
    eng = _engine(rsa, nd, params, 1 << 20)
    try:
        got, tot = eng.hops(N.HEARS, [0])
        label = np.full(nd.n, -1, dtype=np.int32)
        label[0] = 0
        level = np.array([0], dtype=np.int32)
        L = 0
        while len(level):
            d = DeviceArray(level)
            t0 = 10 * AIR * L
            eng.tick_run_sources_device(t0, t0 + TICK, d.ptr.value, len(level), t0, AIR)
            res = eng.result_copy(len(level), cap=1 << 18)
            d.free()
            nxt = np.unique(res.dst)
            nxt = nxt[label[nxt] == -1].astype(np.int32)
            label[nxt] = L + 1
            level, L = nxt, L + 1
        np.testing.assert_array_equal(got["hop"], label)
        assert tot["max_hop"] == L - 1 > 5 and tot["reached"] == (label >= 0).sum() > 200
    finally:
        eng.close()


# ---- 7. read-only -------------------------------------------------------------------------------------------------------------

def _same_result(a, b, what):
    assert a.count == b.count, (what, a.count, b.count)
    for f in ("pkt", "dst", "verdict", "pkt_interference", "pkt_offset"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg="%s: %s" % (what, f))
    np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr), err_msg=what + ": sinr")


def _asker(a):
    def ask():
        for d in H.DIRS:
            a.hops(d, [0, 5])
        a.hops(N.HEARS, [7], -85.0, fields=())
    return ask


def test_a_query_leaves_the_generator_alone(rsa, O):
    """a lone tick whose verdicts are drawn from java.util.Random (fractional rxprob) gives the same bits and leaves the same
    generator state with queries around it as on a context that never queried"""
    nd0, params, _ = N.scene("n300_shadow")
    nd = N._copy(nd0)
    nd.rxprob[::5] = 0.6
    a, b = _engine(rsa, nd, params, 1 << 20), _engine(rsa, nd, params, 1 << 20)
    srcs = np.arange(0, nd.n, 7, dtype=np.int32)
    d = DeviceArray(srcs)
    try:
        ask, out = _asker(a), []
        for e in (a, b):
            e.seed(9)
            if e is a:
                ask()
            s0 = e.rng_state
            e.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, AIR)
            if e is a:
                ask()
            out.append((e.result_copy(len(srcs), cap=1 << 18), s0, e.rng_state))
        _same_result(out[0][0], out[1][0], "lone tick")
        assert out[0][1:] == out[1][1:] and out[0][1] != out[0][2]
        assert len(set(out[0][0].verdict.tolist())) == 2
    finally:
        d.free()
        a.close()
        b.close()


def test_a_query_changes_nothing(rsa, O):
    """a plain batch, a channel-energy query (the on-air window) and a CSMA-CA batch on the SINR medium give the same bits with
    queries in front of them as on a context that never queried; E11 / E14 tables, E13's missed table and E15's schedules are
    unchanged by a query; E16 answers the same behind one"""
    nd, params, found = N.scene("n300_shadow_sinr")
    a, b = _engine(rsa, nd, params, 1 << 20), _engine(rsa, nd, params, 1 << 20)
    keep = []
    try:
        rng = np.random.default_rng(2)
        lists = [np.sort(rng.choice(nd.n, 40, replace=False)).astype(np.int32) for _ in range(4)]
        starts = [TICK * k for k in range(4)]
        sched = np.zeros((nd.n, 3), dtype=np.int64)
        sched[::3] = (1000, 400, 500)   # (asleep when the frames of these ticks begin)
        rows = np.full((nd.n, 4), -1, dtype=np.int32)
        rows[:, 0] = (np.arange(nd.n) + 1) % nd.n
        traffic = np.zeros((nd.n, 4), dtype=np.int64)
        traffic[::2, 0] = 700
        for e in (a, b):
            e.stats_enable()
            e.listen_set(sched)
            e.linkstats_enable(4)
            e.linkstats_watch(rows)
            e.traffic_set(traffic)
        ask = _asker(a)

        def both(fn):
            ask()
            ra, rb = fn(a), fn(b)
            ask()
            return ra, rb

        def batch(e):
            arrs = [DeviceArray(s) for s in lists]
            keep.extend(arrs)
            e.batch_run_sources_device(starts, [t + TICK for t in starts], [x.ptr.value for x in arrs], [len(s) for s in lists], starts, [AIR] * 4)
            return [e.batch_result_copy(k, len(lists[k]), cap=1 << 18) for k in range(4)]

        for k, (x, y) in enumerate(zip(*both(batch))):
            _same_result(x, y, "batch slot %d" % k)
        ea, eb = both(lambda e: e.channel_energy(3 * TICK + 500, cca_threshold_dbm=-90.0))
        np.testing.assert_array_equal(_bits(ea[0]), _bits(eb[0]))
        np.testing.assert_array_equal(ea[1], eb[1])
        assert (ea[1] != 0).any()

        def csma(e):
            t0 = [30 * TICK + s for s in starts]
            return e.batch_run_sources_csma(t0, [t + TICK for t in t0], lists, t0, [AIR] * 4, t0, -85.0, rsa.Engine.csma_params(seed=3))

        (ca, na), (cb, nb) = both(csma)
        np.testing.assert_array_equal(na, nb)
        for f in ca:
            np.testing.assert_array_equal(np.asarray(ca[f]).view(np.uint8), np.asarray(cb[f]).view(np.uint8), err_msg="csma " + f)

        def tables(e):
            return (e.stats_read()[0].tobytes(), e.stats_read()[1], e.listen_missed().tobytes(), e.linkstats_read()[0].tobytes(),
                    e.linkstats_read()[1], e.linkstats_peers().tobytes(), e.traffic_get().tobytes())

        ta = tables(a)
        ask()
        assert tables(a) == ta == tables(b)
        assert np.frombuffer(ta[3], dtype=LK.DTYPE)["heard"].sum() > 0 and np.frombuffer(ta[2], dtype=np.uint64).sum() > 0
        for d in H.DIRS:
            N.same(a.neighbors(d, 8), N.rows(nd, params, d, 8, None, found[d]), "E16 behind a hop query, dir=%d" % d)
    finally:
        for d in keep:
            d.free()
        a.close()
        b.close()


# ---- 8. refusals, each with nothing launched; device lists --------------------------------------------------------------------

def _refused(eng, code, fn):
    with pytest.raises(Exception) as e:
        fn()
    assert getattr(e.value, "code", None) == code, e.value
    assert _hop_kernels(eng) == set(), _hop_kernels(eng)


def test_refusals(rsa, O):
    import ctypes as C
    nd, params, _ = N.scene("n65")
    eng = _engine(rsa, nd, params)
    hop = DeviceArray(np.zeros(nd.n, dtype=np.int32))
    root = DeviceArray(np.zeros(4, dtype=np.int32))
    try:
        eng.profile_enable(1)
        L, h = eng._L, eng._h
        st = rsa.HopsOut(hop=hop.ptr.value)
        q = lambda *a: rsa._lib.check(L.rm_hops_query_device(*a))
        _refused(eng, INVALID, lambda: q(None, 0, -90.0, root.ptr.value, 1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, 0, -90.0, root.ptr.value, 1, None, None))
        _refused(eng, INVALID, lambda: q(h, 0, -90.0, root.ptr.value, 1, C.byref(rsa.HopsOut()), None))
        _refused(eng, INVALID, lambda: rsa._lib.check(L.rm_hops_query(h, 0, -90.0, root.ptr.value, 1, C.byref(rsa.HopsOut()), None)))
        for d in (-1, 2):
            _refused(eng, INVALID, lambda: eng.hops(d, [0]))
            _refused(eng, INVALID, lambda: q(h, d, -90.0, root.ptr.value, 1, C.byref(st), None))
        _refused(eng, INVALID, lambda: eng.hops(N.HEARS, [0], float("nan")))
        _refused(eng, INVALID, lambda: q(h, 1, float("nan"), root.ptr.value, 1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, 1, -90.0, root.ptr.value, -1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, 1, -90.0, None, 1, C.byref(st), None))
        for bad in ([0, -1], [nd.n], [3, -2 ** 31]):
            _refused(eng, INVALID, lambda: eng.hops(N.HEARD_BY, bad))
        eng.tick_begin(0, TICK)
        _refused(eng, STATE, lambda: eng.hops(N.HEARS, [0]))
        eng.enqueue_tx(1, 0, AIR)
        eng.tick_flush(cap=1 << 12)
        eng.set_partition(0, nd.n // 2)
        _refused(eng, STATE, lambda: eng.hops(N.HEARS, [0]))
        eng.set_partition(0, nd.n)
        eng.set_partition_spatial(0, 2)
        _refused(eng, STATE, lambda: eng.hops(N.HEARD_BY, [0]))
        eng.set_partition_spatial(0, 1)
        for kind in (0, 1, 2, 3):
            eng.set_model(kind)
            _refused(eng, STATE, lambda: eng.hops(N.HEARD_BY, [0]))
            _refused(eng, STATE, lambda: q(h, 0, -90.0, root.ptr.value, 1, C.byref(st), None))
        eng.set_model(4)
        # the gather's refusals
        for args in ((None, hop.ptr.value, root.ptr.value, 4, root.ptr.value), (h, hop.ptr.value, root.ptr.value, -1, root.ptr.value),
                     (h, None, root.ptr.value, 4, root.ptr.value), (h, hop.ptr.value, None, 4, root.ptr.value), (h, hop.ptr.value, root.ptr.value, 4, None)):
            _refused(eng, INVALID, lambda: rsa._lib.check(L.rm_hops_next_device(*args)))
        assert eng.hops(N.HEARD_BY, [])[1] == {"reached": 0, "max_hop": -1, "roots": 0}   # n_roots == 0 is RM_OK
        assert eng.hops(N.HEARD_BY, [0])[0]["hop"].shape == (nd.n,) and _hop_kernels(eng) != set()
    finally:
        hop.free()
        root.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import radio_sim_amd as rsa
eng = rsa.Engine(0)
try:
    eng.upload_nodes(np.zeros(4), np.arange(4.0))
    eng.set_model(4)
    eng.profile_enable(1)
    try:
        eng.hops(rsa.NB_HEARS, [0])
    except rsa.RadioMediumError as e:
        assert e.code == -5 and "RM_GRAPH" in str(e), e
        assert not [k for k in eng.profile_kernels() if k.startswith("k_hop_") or k.startswith("k_nb_")]
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_query_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)


def test_device_roots_outside_the_table(rsa, O):
    """-1, n_nodes, INT32_MIN and INT32_MAX in a device root list are ignored; the others count, duplicates once"""
    nd, params, found = N.scene("n300")
    eng = _engine(rsa, nd, params)
    try:
        roots = np.array([7, -1, 8, nd.n, -2 ** 31, 299, 2 ** 31 - 1, 7], dtype=np.int32)
        for d in H.DIRS:
            want = H.tree(nd.n, found[d], roots)
            assert want["totals"]["roots"] == 3
            H.same(*_device_query(eng, d, roots, nd.n), want, "dir=%d" % d)
            H.same(*_device_query(eng, d, np.array([-1, nd.n], dtype=np.int32), nd.n), H.tree(nd.n, found[d], []), "dir=%d, no valid root" % d)
    finally:
        eng.close()


# ---- 9. the chain: traffic rows -> want -> unicast outcomes; the parents as a watch table --------------------------------------

def test_chain(rsa, O):
    """hops_next_device over E15's generated rows equals the numpy gather; handed to rm_unicast_query_device after a batch over the
    same rows it gives the statuses unicast_ref gives for want = parent[src]; the parent array is a valid K = 1 watch table"""
    nd, params, found = N.scene("n300_shadow")
    eng = _engine(rsa, nd, params, 1 << 20)
    n_ticks, cap = 4, 64   # (60 sources a tick: every row ends in padding)
    tb = [TICK * k for k in range(n_ticks)]
    te = [t + TICK for t in tb]
    keep = []

    def dev(a):
        keep.append(DeviceArray(a))
        return keep[-1].ptr.value

    try:
        want_tree = H.tree(nd.n, found[N.HEARD_BY], [0])
        d_hop, d_par = dev(np.zeros(nd.n, dtype=np.int32)), dev(np.zeros(nd.n, dtype=np.int32))
        d_root = dev(np.array([0], dtype=np.int32))
        eng.hops_device(N.HEARD_BY, d_root, 1, d_hop, d_par)
        parent = DeviceArray.read(d_par, np.int32, nd.n)
        np.testing.assert_array_equal(parent, want_tree["parent"])
        # E15: every fifth node sends once per tick
        table = np.zeros((nd.n, 4), dtype=np.int64)
        table[::5] = (TICK, 100, 0, 0)
        eng.traffic_set(table)
        d_src, d_cnt = dev(np.zeros(n_ticks * cap, dtype=np.int32)), dev(np.zeros(n_ticks, dtype=np.int32))
        d_want = dev(np.full(n_ticks * cap + 8, -777, dtype=np.int32))
        eng.traffic_generate_device(5, tb, te, cap, d_src, d_cnt)
        eng.hops_next_device(d_par, d_src, n_ticks * cap, d_want)
        eng.sync()
        src = DeviceArray.read(d_src, np.int32, n_ticks * cap)
        got_want = DeviceArray.read(d_want, np.int32, n_ticks * cap + 8)
        assert (src >= 0).sum() > 100 and (src == -1).sum() > 0 and (got_want[-8:] == -777).all()
        np.testing.assert_array_equal(got_want[:-8], np.where(src >= 0, parent[np.maximum(src, 0)], -1))
        # out-of-table sources give -1
        odd = np.array([3, -1, nd.n, 2 ** 31 - 1, -2 ** 31, 299], dtype=np.int32)
        d_odd, d_out = dev(odd), dev(np.zeros(len(odd), dtype=np.int32))
        eng.hops_next_device(d_par, d_odd, len(odd), d_out)
        eng.sync()
        assert DeviceArray.read(d_out, np.int32, len(odd)).tolist() == [parent[3], -1, -1, -1, -1, parent[299]]
        # the batch over the padded rows, then "did it reach its parent"
        air = 400   # (every tick's frames end inside their tick)
        eng.batch_run_sources_device(tb, te, [d_src + 4 * b * cap for b in range(n_ticks)], [cap] * n_ticks, tb, [air] * n_ticks)
        outs = {"status": dev(np.full(n_ticks * cap, 99, dtype=np.uint8)), "reply_src": dev(np.full(n_ticks * cap, -5, dtype=np.int32))}
        eng.unicast_query_device([cap] * n_ticks, d_want, dict(outs, link=None, rssi=None, sinr=None))
        eng.sync()
        status = DeviceArray.read(outs["status"], np.uint8, n_ticks * cap).reshape(n_ticks, cap)
        reply = DeviceArray.read(outs["reply_src"], np.int32, n_ticks * cap).reshape(n_ticks, cap)
        mdl = N._model(params)
        seen = set()
        for b in range(n_ticks):
            row = src[b * cap:(b + 1) * cap]
            live = row[row >= 0]
            res = O.tick(mdl, nd, nd.packets(live, start_us=tb[b], air_us=air), cap=len(live) * nd.n + 1)
            exp = U.outcome(nd.n, row, U.offsets(res.pkt, len(live)).tolist() + [int(res.count)] * (cap - len(live)), res.dst, res.verdict,
                            res.rssi, None, got_want[b * cap:(b + 1) * cap])
            np.testing.assert_array_equal(status[b], exp["status"], err_msg="tick %d: status" % b)
            np.testing.assert_array_equal(reply[b], exp["reply_src"], err_msg="tick %d: reply_src" % b)
            seen |= set(exp["status"].tolist())
        assert {U.DELIVERED, 0} <= seen   # (a node whose parent heard it; padding and the root's own frame ask nothing)
        # the parents as a K = 1 watch table
        eng.linkstats_enable(1)
        eng.linkstats_watch_device(d_par)
        np.testing.assert_array_equal(eng.linkstats_peers().reshape(-1), want_tree["parent"])
    finally:
        for d in keep:
            d.free()
        eng.close()
