"""The route query (rm_routes_*, rm_routes.hip) on the GPU.  Expected routes come from the oracle's
potential links and the error model's reference through tests/routes_ref.py alone (tests/test_routes_ref.py holds the scenes'
conditions for that reference).  Every comparison is exact: equal integers, equal rssi bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hops_ref as H
import neighbors_ref as N
import routes_ref as R
import test_gpu_hops as TH
from test_gpu_cca import _bits, _engine
from util import DeviceArray

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5
TICK, AIR = 1000, 4256
OPTIONAL = ("parent", "rssi", "link_cost", "children")
FIELDS = (("cost", np.uint64), ("parent", np.int32), ("rssi", np.float64), ("link_cost", np.uint32), ("children", np.int32))
Q = {k: v[0] for k, v in R.SETS.items()}


def _p(rsa, q, d, **kw):
    return rsa.Engine.routes_params(direction=d, **dict(q, **kw))


def _route_kernels(eng):
    return {k for k in eng.profile_kernels() if k.startswith("k_route_") or k.startswith("k_nb_") or k.startswith("k_hop_")}


def _paths(eng):
    """which walking kernels ran: {"boxes", "scan"}"""
    names = [k for k in _route_kernels(eng) if k.startswith("k_route_relax") or k.startswith("k_route_parent")]
    return {"scan" if k.replace(" ", "").endswith("true>") else "boxes" for k in names}


def _device_query(eng, params, roots, n, leave_out=()):
    """the device form into buffers filled with a pattern -> (outputs, totals) as the host form returns them"""
    dt = dict(FIELDS)
    bufs = {f: DeviceArray(np.full(n, 0x5A5A5A5A if f != "rssi" else 7.0, dtype=dt[f])) for f in dt if f not in leave_out}
    dr = DeviceArray(np.ascontiguousarray(roots, dtype=np.int32)) if len(roots) else None
    try:
        ptr = {f: (bufs[f].ptr.value if f in bufs else None) for f in dt}
        tot = eng.routes_device(params, dr.ptr.value if dr else None, len(roots), ptr["cost"], ptr["parent"], ptr["rssi"], ptr["link_cost"], ptr["children"])
        return {f: DeviceArray.read(bufs[f].ptr.value, dt[f], n) for f in bufs}, tot
    finally:
        for d in list(bufs.values()) + [dr]:
            if d is not None:
                d.free()


# ---- 1. against the reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pset", list(R.SETS))
@pytest.mark.parametrize("name", list(N.SCENES))
def test_routes_against_the_reference(rsa, O, name, pset):
    """both directions, the tests' root sets, a threshold and another cap, host and device forms, every optional output NULL in
    turn.  Tables of up to 64 nodes are not sorted (the whole-table scan); the larger ones walk the boxes."""
    nd, params, found = R.scene(name, pset)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in R.DIRS:
            for label, roots in H.root_sets(nd, name).items():
                for kw in ({}, {"min_rssi_dbm": -85.0}, {"max_link_cost": 300}, {"min_rssi_dbm": R.INF}) if label in ("0", "0,S", "all") else ({},):
                    q = dict(Q[pset], **kw)
                    what = "%s %s dir=%d roots=%s %s" % (name, pset, d, label, kw)
                    want = R.tree(nd.n, found[d], roots, q)
                    R.same(*eng.routes(_p(rsa, q, d), roots), want, what + ", host")
                    if not kw:
                        R.same(*_device_query(eng, _p(rsa, q, d), roots, nd.n), want, what + ", device")
            prm = _p(rsa, Q[pset], d)
            want = R.tree(nd.n, found[d], [0], Q[pset])
            for out in OPTIONAL:
                got, tot = _device_query(eng, prm, [0], nd.n, leave_out=(out,))
                assert set(got) == {"cost"} | set(OPTIONAL) - {out}
                R.same(got, tot, want, "%s %s dir=%d device without %s" % (name, pset, d, out))
                got, tot = eng.routes(prm, [0], fields=(out,))
                assert set(got) == {"cost", out}
                R.same(got, tot, want, "%s %s dir=%d host with %s alone" % (name, pset, d, out))
            R.same(*_device_query(eng, prm, [0], nd.n, leave_out=OPTIONAL), want, "%s %s dir=%d device, cost alone" % (name, pset, d))
        assert _paths(eng) == ({"scan"} if nd.n <= 64 else {"boxes"}), _route_kernels(eng)
    finally:
        eng.close()


# ---- 2. ladders: every node is labelled too high first and lowered later -------------------------------------------------------

@pytest.mark.parametrize("name, path", [("ladder40", "scan"), ("ladder70", "boxes")])
def test_ladders(rsa, O, name, path):
    q = Q["MARGINAL"]
    nd, params, found = R.scene(name, "MARGINAL")
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in R.DIRS:
            for roots in ([0], [nd.n - 1], [nd.n // 2], [0, nd.n - 1]):
                got, tot = eng.routes(_p(rsa, q, d), roots)
                R.same(got, tot, R.tree(nd.n, found[d], roots, q), "%s dir=%d roots=%s" % (name, d, roots))
            got, tot = eng.routes(_p(rsa, q, d), [0])
            assert tot == {"reached": nd.n, "roots": 1, "max_cost": 128 * (nd.n - 1)} and got["parent"].tolist() == list(range(-1, nd.n - 1))
            assert eng.hops(d, [0])[1]["max_hop"] == nd.n // 2   # (the hop query skips: the first labels were the two-step links')
        assert _paths(eng) == {path}, _route_kernels(eng)
    finally:
        eng.close()


# ---- 3. frontiers that span many workgroups -----------------------------------------------------------------------------------

def test_n3000(rsa, O):
    """rich(3000, 5) under MARGINAL: three boxes of 1024 receivers, frontiers of hundreds of nodes, many re-labelled nodes"""
    q = Q["MARGINAL"]
    nd, params, found = R.scene("n3000_shadow", "MARGINAL")
    sp = N.special(nd)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in R.DIRS:
            for roots, kw in (([0], {}), ([0], {"min_rssi_dbm": -100.0}), ([sp["A"], sp["B"], 17, 17], {})):
                qq = dict(q, **kw)
                R.same(*eng.routes(_p(rsa, qq, d), roots), R.tree(nd.n, found[d], roots, qq), "n3000 dir=%d roots=%s %s" % (d, roots, kw))
            want = R.tree(nd.n, found[d], [0], q)
            h = H.tree(nd.n, found[d], [0])
            assert (R.depth(want) > h["hop"]).sum() > 500 and want["totals"]["reached"] > 2800
            R.same(*_device_query(eng, _p(rsa, q, d), [0], nd.n), want, "n3000 dir=%d device" % d)
        assert _paths(eng) == {"boxes"}
    finally:
        eng.close()


# ---- 4. 65 537 nodes: 65 boxes, the second round of the box loop ----------------------------------------------------------------

def test_large_table_none_is_the_hop_query(rsa, O):
    """RM_EM_NONE: cost = 128 * hop, and parent, rssi bits and children are rm_hops_query's on the same context"""
    nd, _ = N.large(65537)
    sp = N.special(nd)
    eng = _engine(rsa, nd, N.SHADOW)
    try:
        for d in R.DIRS:
            h, ht = eng.hops(d, [0, sp["S"]])
            got, tot = eng.routes(_p(rsa, Q["NONE"], d), [0, sp["S"]])
            assert ht["reached"] > 1000 and ht["max_hop"] > 10   # (not vacuous)
            np.testing.assert_array_equal(got["cost"], np.where(h["hop"] >= 0, 128 * h["hop"].astype(np.int64), -1).astype(np.uint64))
            np.testing.assert_array_equal(got["parent"], h["parent"])
            np.testing.assert_array_equal(_bits(got["rssi"]), _bits(h["rssi"]))
            np.testing.assert_array_equal(got["children"], h["children"])
            np.testing.assert_array_equal(got["link_cost"], np.where(h["hop"] >= 1, 128, 0).astype(np.uint32))
            assert tot == {"reached": ht["reached"], "roots": 2, "max_cost": 128 * ht["max_hop"]}
    finally:
        eng.close()


def test_large_table_marginal_certificate(rsa, O):
    """MARGINAL at 65 537 nodes, too large for the oracle: the answer is held to a certificate computed with numpy.  The costs are
    attained (cost[j] == cost[parent[j]] + link_cost[j], link_cost[j] the reference's cost of rssi[j]); and for every node whose
    E16 degree is at most 16 the row is the node's whole link set, so no row entry may lower its cost or precede its parent at
    equal cost.  E16's tests hold E16 to the oracle at this size."""
    q = Q["MARGINAL"]
    nd, _ = N.large(65537)
    sp = N.special(nd)
    eng = _engine(rsa, nd, dict(N.SHADOW, **R.SETS["MARGINAL"][1]))
    big = np.int64(1) << 60   # "no cost": larger than every path cost, small enough to add to
    try:
        for d in R.DIRS:
            nb = eng.neighbors(d, 16)
            got, tot = eng.routes(_p(rsa, q, d), [0, sp["S"]])
            unreached = got["cost"] == R.UNREACHED
            cost = np.where(unreached, big, got["cost"].astype(np.int64))
            parent, lc = got["parent"].astype(np.int64), got["link_cost"].astype(np.int64)
            assert tot == {"reached": int((~unreached).sum()), "roots": 2, "max_cost": int(cost[~unreached].max())}
            assert cost[0] == 0 and cost[sp["S"]] == 0 and cost[sp["A"]] == 128 and unreached[sp["LONE"]]
            has = parent >= 0
            np.testing.assert_array_equal(has, ~unreached & (cost > 0))
            assert has.sum() > 1000 and (lc[has] > 128).sum() > 100 and tot["max_cost"] > 10 * 128   # (not vacuous)
            np.testing.assert_array_equal(cost[has], cost[parent[has]] + lc[has])
            np.testing.assert_array_equal(lc[has], R.link_costs_np(q, got["rssi"][has]))
            assert (lc[~has] == 0).all() and (_bits(got["rssi"])[~has] == N.NAN_BITS).all()
            np.testing.assert_array_equal(got["children"], np.bincount(parent[has], minlength=nd.n))
            # the rows of the nodes whose whole link set they are
            whole = nb["degree"] <= 16
            peer = nb["peer"].astype(np.int64)
            valid = peer >= 0
            rc = R.link_costs_np(q, np.where(valid, nb["rssi"], -R.INF).reshape(-1)).reshape(peer.shape)
            counts = valid & (rc >= 0)
            via = np.where(counts, cost[np.where(valid, peer, 0)] + rc, big)       # the cost through each row entry
            via = np.where(via >= big, big, via)
            rows = whole & ~(got["cost"] == 0)
            assert (whole & has).sum() > 1000 and (whole & unreached).sum() > 0
            assert (via[rows] >= cost[rows][:, None]).all()                           # nothing could be lowered; the unreached stay out
            assert (via[whole & has].min(axis=1) == cost[whole & has]).all()                 # and every cost is attained in the row
            first = np.argmax(via == cost[:, None], axis=1)                          # E16's order: the first equal-cost entry
            pick = np.flatnonzero(whole & has)
            np.testing.assert_array_equal(parent[pick], peer[pick, first[pick]])
            np.testing.assert_array_equal(_bits(got["rssi"])[pick], _bits(nb["rssi"])[pick, first[pick]])
            assert ((via == cost[:, None])[pick].sum(axis=1) > 1).sum() > 20        # (ties between candidates occur)
    finally:
        eng.close()


# ---- 5. every state of the table ----------------------------------------------------------------------------------------------

def _check_all(rsa, eng, nd, params, what, sp):
    q = Q["MARGINAL"]
    for d in R.DIRS:
        found = N.links(nd, params, d)
        for roots, kw in (([0], {}), ([sp["S"], 5], {}), ([0], {"min_rssi_dbm": -99.0})):
            qq = dict(q, **kw)
            R.same(*eng.routes(_p(rsa, qq, d), roots), R.tree(nd.n, found, roots, qq), "%s dir=%d roots=%s %s" % (what, d, roots, kw))


def test_after_node_changes(rsa, O):
    """a node moved out of its group's box (rm_node_update, rm_nodes_move); one far node's txpower raised until other nodes hear it;
    radios switched off and on; another noise floor; a node moved outside the fp32 frame (the whole-table scan answers)"""
    nd0, params, _ = R.scene("n300_shadow", "MARGINAL")
    nd, sp = N._copy(nd0), N.special(nd0)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        _check_all(rsa, eng, nd, params, "before", sp)
        TH._update(eng, nd, 3, x=nd.x[sp["S"]] + 2.0, y=nd.y[sp["S"]] + 1.0)      # from the field to the crafted nodes
        _check_all(rsa, eng, nd, params, "rm_node_update: moved far", sp)
        nd.x[[10, 11]], nd.y[[10, 11]] = [nd.x[sp["LONE"]] + 10.0, -300.0], [nd.y[sp["LONE"]], -300.0]
        eng.move_nodes(np.array([10, 11], dtype=np.int32), nd.x[[10, 11]], nd.y[[10, 11]])
        _check_all(rsa, eng, nd, params, "rm_nodes_move", sp)
        TH._update(eng, nd, sp["LONE"], txpower=75.0)                             # 5 km and more away: now heard by the crafted nodes
        for d in R.DIRS:
            want = R.tree(nd.n, N.links(nd, params, d), [sp["LONE"]], Q["MARGINAL"])
            assert want["totals"]["reached"] > 5 or d == R.HEARD_BY
            R.same(*eng.routes(_p(rsa, Q["MARGINAL"], d), [sp["LONE"]]), want, "the loud lone root dir=%d" % d)
        _check_all(rsa, eng, nd, params, "txpower raised", sp)
        TH._update(eng, nd, sp["A"], enabled=0)
        TH._update(eng, nd, sp["OFF"], enabled=1)
        TH._update(eng, nd, 0, enabled=0)                                         # (a root is a root whatever its radio state)
        _check_all(rsa, eng, nd, params, "radios switched", sp)
        assert _paths(eng) == {"boxes"}
        TH._update(eng, nd, 20, x=4.0e7, y=-3.0e7)
        _check_all(rsa, eng, nd, params, "outside the fp32 frame", sp)
        assert _paths(eng) == {"boxes", "scan"}
    finally:
        eng.close()


def test_both_kernel_paths(rsa, O):
    """the same scene through the boxes and through the whole-table scan (a far node makes the fp32 frame too coarse for the boxes;
    it hears nobody and nobody hears it): equal bits, and rm_profile_kernels tells which ran"""
    nd0, params, found = R.scene("n300_shadow", "MARGINAL")
    nd = N._copy(nd0)
    sp = N.special(nd)
    cases = [(d, kw) for d in R.DIRS for kw in ({}, {"min_rssi_dbm": -99.0})]
    out = {}
    for path in ("boxes", "scan"):
        eng = _engine(rsa, nd, params)
        try:
            eng.profile_enable(1)
            if path == "scan":
                TH._update(eng, nd, sp["LONE"], x=5.0e7, y=5.0e7)
            out[path] = [eng.routes(_p(rsa, dict(Q["MARGINAL"], **kw), d), [0, sp["S"]]) for d, kw in cases]
            assert _paths(eng) == {path}, _route_kernels(eng)
            assert {"k_nb_prep", "k_route_init", "k_route_seed", "k_route_totals"} <= _route_kernels(eng)
            assert not [k for k in _route_kernels(eng) if k.startswith("k_hop_")]
        finally:
            eng.close()
    for k, (d, kw) in enumerate(cases):
        (a, ta), (b, tb) = out["boxes"][k], out["scan"][k]
        R.same(a, ta, R.tree(nd0.n, found[d], [0, sp["S"]], dict(Q["MARGINAL"], **kw)), "boxes dir=%d %s" % (d, kw))
        R.same(b, tb, R.tree(nd0.n, found[d], [0, sp["S"]], dict(Q["MARGINAL"], **kw)), "scan dir=%d %s" % (d, kw))


def test_permuted_roots_give_the_same_answer(rsa, O):
    nd, params, found = R.scene("n300_shadow", "MARGINAL")
    eng = _engine(rsa, nd, params)
    try:
        roots = np.array([0, 17, 123, 250, 17, N.special(nd)["S"]], dtype=np.int32)
        for d in R.DIRS:
            a, ta = eng.routes(_p(rsa, Q["MARGINAL"], d), roots)
            b, tb = eng.routes(_p(rsa, Q["MARGINAL"], d), roots[::-1].copy())
            c, tc = _device_query(eng, _p(rsa, Q["MARGINAL"], d), np.random.default_rng(5).permutation(roots), nd.n)
            assert ta == tb == tc
            for f, _ in FIELDS:
                assert a[f].tobytes() == b[f].tobytes() == c[f].tobytes(), (d, f)
            R.same(a, ta, R.tree(nd.n, found[d], roots, Q["MARGINAL"]), "dir=%d" % d)
    finally:
        eng.close()


# ---- 6. the rule's snr is the SINR medium's sinr with nothing else on the air ---------------------------------------------------

def test_snr_is_the_sinr_of_a_lone_frame(rsa, O):
    """lone single-source ticks on n300_sinr: every heard link's sinr column is, bit for bit, rssi - 10 * det_log10(ld_noise_lin) --
    the value the reference's link cost starts from"""
    nd, params, _ = N.scene("n300_sinr")
    eng = _engine(rsa, nd, params, 1 << 20)
    try:
        seen = 0
        for k, s in enumerate((0, 5, 123, N.special(nd)["LOUD"])):
            d = DeviceArray(np.array([s], dtype=np.int32))
            t0 = 20 * AIR * k   # (the frame before has left the air)
            eng.tick_run_sources_device(t0, t0 + TICK, d.ptr.value, 1, t0, AIR)
            res = eng.result_copy(1, cap=1 << 12)
            d.free()
            assert res.count > 0
            np.testing.assert_array_equal(_bits(res.sinr), _bits(np.array([r - R.noise_db() for r in res.rssi.tolist()])))
            seen += int(res.count)
        assert seen > 20
    finally:
        eng.close()


# ---- 7. read-only -------------------------------------------------------------------------------------------------------------

def _asker(a):
    import radio_sim_amd as rsa

    def ask():
        for d in R.DIRS:
            a.routes(_p(rsa, Q["OQPSK"], d), [0, 5])
        a.routes(_p(rsa, Q["NONE"], R.HEARS, min_rssi_dbm=-85.0), [7], fields=())
    return ask


def test_a_query_leaves_the_generator_alone(rsa, O, monkeypatch):
    """the hop query's test with route queries around the tick"""
    monkeypatch.setattr(TH, "_asker", _asker)
    TH.test_a_query_leaves_the_generator_alone(rsa, O)


def test_a_query_changes_nothing(rsa, O, monkeypatch):
    """the hop query's test with route queries in front of the batch, the channel-energy query and the CSMA-CA batch and behind the
    tables' reads"""
    monkeypatch.setattr(TH, "_asker", _asker)
    TH.test_a_query_changes_nothing(rsa, O)


def test_the_hop_query_is_left_alone(rsa, O):
    """E17 answers the same behind a route query, and the route query the same behind E17 and E16"""
    nd, params, found = R.scene("n300_shadow", "MARGINAL")
    eng = _engine(rsa, nd, params)
    try:
        for d in R.DIRS:
            want_h, want_r = H.tree(nd.n, found[d], [0, 9]), R.tree(nd.n, found[d], [0, 9], Q["MARGINAL"])
            H.same(*eng.hops(d, [0, 9]), want_h, "before")
            R.same(*eng.routes(_p(rsa, Q["MARGINAL"], d), [0, 9]), want_r, "between")
            H.same(*eng.hops(d, [0, 9]), want_h, "behind")
            eng.neighbors(d, 4)
            R.same(*eng.routes(_p(rsa, Q["MARGINAL"], d), [0, 9]), want_r, "behind E17 and E16")
    finally:
        eng.close()


# ---- 8. refusals, each with nothing launched; device lists --------------------------------------------------------------------

def _refused(eng, code, fn):
    with pytest.raises(Exception) as e:
        fn()
    assert getattr(e.value, "code", None) == code, e.value
    assert _route_kernels(eng) == set(), _route_kernels(eng)


def test_refusals(rsa, O):
    import ctypes as C
    nd, params, _ = N.scene("n65")
    eng = _engine(rsa, nd, params)
    cost = DeviceArray(np.zeros(nd.n, dtype=np.uint64))
    root = DeviceArray(np.zeros(4, dtype=np.int32))
    try:
        eng.profile_enable(1)
        L, h = eng._L, eng._h
        st = rsa.RoutesOut(cost=cost.ptr.value)
        ok = _p(rsa, Q["OQPSK"], 0)
        q = lambda *a: rsa._lib.check(L.rm_routes_query_device(*a))
        _refused(eng, INVALID, lambda: q(None, C.byref(ok), root.ptr.value, 1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, None, root.ptr.value, 1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), root.ptr.value, 1, None, None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), root.ptr.value, 1, C.byref(rsa.RoutesOut()), None))
        _refused(eng, INVALID, lambda: rsa._lib.check(L.rm_routes_query(h, C.byref(ok), root.ptr.value, 1, C.byref(rsa.RoutesOut()), None)))
        bad = ({"direction": -1}, {"direction": 2}, {"kind": 2}, {"kind": -1}, {"reserved": 1}, {"us_per_bit": 0.0}, {"us_per_bit": -4.0},
               {"us_per_bit": R.INF}, {"us_per_bit": float("nan")}, {"air_us": -1}, {"min_rssi_dbm": float("nan")}, {"max_link_cost": 127},
               {"max_link_cost": 65536})
        for kw in bad:
            prm = rsa.Engine.routes_params(**dict(dict(Q["OQPSK"], direction=0), **kw))
            _refused(eng, INVALID, lambda: eng.routes(prm, [0]))
            _refused(eng, INVALID, lambda: q(h, C.byref(prm), root.ptr.value, 1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), root.ptr.value, -1, C.byref(st), None))
        _refused(eng, INVALID, lambda: q(h, C.byref(ok), None, 1, C.byref(st), None))
        for roots in ([0, -1], [nd.n], [3, -2 ** 31]):
            _refused(eng, INVALID, lambda: eng.routes(ok, roots))
        eng.tick_begin(0, TICK)
        _refused(eng, STATE, lambda: eng.routes(ok, [0]))
        eng.enqueue_tx(1, 0, AIR)
        eng.tick_flush(cap=1 << 12)
        eng.set_partition(0, nd.n // 2)
        _refused(eng, STATE, lambda: eng.routes(ok, [0]))
        eng.set_partition(0, nd.n)
        eng.set_partition_spatial(0, 2)
        _refused(eng, STATE, lambda: eng.routes(ok, [0]))
        eng.set_partition_spatial(0, 1)
        for kind in (0, 1, 2, 3):
            eng.set_model(kind)
            _refused(eng, STATE, lambda: eng.routes(ok, [0]))
            _refused(eng, STATE, lambda: q(h, C.byref(ok), root.ptr.value, 1, C.byref(st), None))
        eng.set_model(4)
        assert eng.routes(ok, [])[1] == {"reached": 0, "roots": 0, "max_cost": 0}   # n_roots == 0 is RM_OK
        assert eng.routes(_p(rsa, Q["OQPSK"], 0, max_link_cost=128), [0])[1]["reached"] > 1   # the smallest cap is accepted
        assert eng.routes(_p(rsa, Q["OQPSK"], 0, max_link_cost=65535), [0])[0]["cost"].shape == (nd.n,) and _route_kernels(eng) != set()
    finally:
        cost.free()
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
        eng.routes(rsa.Engine.routes_params(rsa.NB_HEARS), [0])
    except rsa.RadioMediumError as e:
        assert e.code == -5 and "RM_GRAPH" in str(e), e
        assert not [k for k in eng.profile_kernels() if k.startswith("k_route_") or k.startswith("k_nb_")]
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
    nd, params, found = R.scene("n300", "MARGINAL")
    eng = _engine(rsa, nd, params)
    try:
        roots = np.array([7, -1, 8, nd.n, -2 ** 31, 299, 2 ** 31 - 1, 7], dtype=np.int32)
        for d in R.DIRS:
            want = R.tree(nd.n, found[d], roots, Q["MARGINAL"])
            assert want["totals"]["roots"] == 3
            R.same(*_device_query(eng, _p(rsa, Q["MARGINAL"], d), roots, nd.n), want, "dir=%d" % d)
            R.same(*_device_query(eng, _p(rsa, Q["MARGINAL"], d), np.array([-1, nd.n], dtype=np.int32), nd.n), R.tree(nd.n, found[d], [], Q["MARGINAL"]),
                   "dir=%d, no valid root" % d)
    finally:
        eng.close()


# ---- 9. the chain: the routes' parents -> want -> unicast outcomes; the parents as a watch table --------------------------------

def test_chain(rsa, O):
    """the route query's parent array through rm_hops_next_device into rm_unicast_query_device after a batch over the same rows:
    the statuses unicast_ref gives for want = parent[src]; and the parent array as a K = 1 watch table"""
    import unicast_ref as U
    q = Q["MARGINAL"]
    nd, params, found = R.scene("n300_shadow", "MARGINAL")
    eng = _engine(rsa, nd, params, 1 << 20)
    n_ticks, cap = 4, 64
    tb = [TICK * k for k in range(n_ticks)]
    te = [t + TICK for t in tb]
    keep = []

    def dev(a):
        keep.append(DeviceArray(a))
        return keep[-1].ptr.value

    try:
        want_tree = R.tree(nd.n, found[R.HEARD_BY], [0], q)
        assert (want_tree["parent"] != H.tree(nd.n, found[R.HEARD_BY], [0])["parent"]).sum() >= 50   # (not the hop query's parents)
        d_cost, d_par = dev(np.zeros(nd.n, dtype=np.uint64)), dev(np.zeros(nd.n, dtype=np.int32))
        d_root = dev(np.array([0], dtype=np.int32))
        eng.routes_device(_p(rsa, q, R.HEARD_BY), d_root, 1, d_cost, d_par)
        parent = DeviceArray.read(d_par, np.int32, nd.n)
        np.testing.assert_array_equal(parent, want_tree["parent"])
        rng = np.random.default_rng(8)
        src = np.full((n_ticks, cap), -1, dtype=np.int32)
        for b in range(n_ticks):
            src[b, :60] = np.sort(rng.choice(nd.n, 60, replace=False))
        d_src = dev(src.reshape(-1))
        d_want = dev(np.full(n_ticks * cap + 8, -777, dtype=np.int32))
        eng.hops_next_device(d_par, d_src, n_ticks * cap, d_want)
        eng.sync()
        got_want = DeviceArray.read(d_want, np.int32, n_ticks * cap + 8)
        flat = src.reshape(-1)
        assert (got_want[-8:] == -777).all()
        np.testing.assert_array_equal(got_want[:-8], np.where(flat >= 0, parent[np.maximum(flat, 0)], -1))
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
            row = src[b]
            live = row[row >= 0]
            res = O.tick(mdl, nd, nd.packets(live, start_us=tb[b], air_us=air), cap=len(live) * nd.n + 1)
            exp = U.outcome(nd.n, row, U.offsets(res.pkt, len(live)).tolist() + [int(res.count)] * (cap - len(live)), res.dst, res.verdict,
                            res.rssi, None, got_want[b * cap:(b + 1) * cap])
            np.testing.assert_array_equal(status[b], exp["status"], err_msg="tick %d: status" % b)
            np.testing.assert_array_equal(reply[b], exp["reply_src"], err_msg="tick %d: reply_src" % b)
            seen |= set(exp["status"].tolist())
        assert {U.DELIVERED, 0} <= seen
        eng.linkstats_enable(1)
        eng.linkstats_watch_device(d_par)
        np.testing.assert_array_equal(eng.linkstats_peers().reshape(-1), want_tree["parent"])
    finally:
        for d in keep:
            d.free()
        eng.close()
