"""The neighbour, hop and route queries (rm_neighbors.hip, rm_hops.hip, rm_routes.hip) on the scenes
of tests/graph_edge_ref.py: a tied three-dimensional lattice that ends on the level, the fp32 slack's edge, aliasing channels with
radios off and non-finite table values, table sizes around the group and the box, root lists of several strides, a hub of degree
K - 1 / K / K + 1, and route costs at their bounds.  Expected values come from the oracle's potential links through
neighbors_ref / hops_ref / routes_ref alone (tests/test_graph_edge_ref.py holds the scenes' conditions for that reference).  Every
comparison is exact: equal integers, equal rssi bits, equal totals."""
import numpy as np
import pytest

import graph_edge_ref as G
import hops_ref as H
import neighbors_ref as N
import routes_ref as R
import test_gpu_hops as TH
import test_gpu_neighbors as TN
import test_gpu_routes as TR
from test_gpu_cca import _bits, _engine
from util import DeviceArray

pytestmark = pytest.mark.gpu

TICK, AIR = 1000, 4256


def _p(rsa, kind, d, **kw):
    return TR._p(rsa, G.Q[kind], d, **kw)


def _all_boxes(eng, path="boxes"):
    """every walking kernel that ran took the one path"""
    for what, paths in (("neighbours", TN._paths(eng)), ("hops", TH._paths(eng)), ("routes", TR._paths(eng))):
        assert paths in (set(), {path}), (what, paths, eng.profile_kernels())


def _neighbours(eng, nd, params, found, d, K, some, what):
    """the all-nodes form and a list form, host and device"""
    want = N.rows(nd, params, d, K, None, found[d])
    part = N.rows(nd, params, d, K, some, found[d])
    N.same(eng.neighbors(d, K), want, what + " all, host")
    N.same(eng.neighbors(d, K, nodes=some), part, what + " list, host")
    N.same(TN._device_query(eng, d, K, None, nd.n), want, what + " all, device")
    N.same(TN._device_query(eng, d, K, some, len(some)), part, what + " list, device")


def _hops(eng, n, d, roots, want, what, min_rssi=-H.INF, device=True, host=True):
    if host:
        H.same(*eng.hops(d, roots, min_rssi), want, what + ", host")
    if device:
        H.same(*TH._device_query(eng, d, roots, n, min_rssi), want, what + ", device")


def _routes(eng, n, prm, roots, want, what, device=True, host=True):
    if host:
        R.same(*eng.routes(prm, roots), want, what + ", host")
    if device:
        R.same(*TR._device_query(eng, prm, roots, n), want, what + ", device")


# ---- 1. lattice3d ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("medium", ["LEVEL", "MARGINAL"])
def test_lattice3d_neighbours(rsa, O, medium):
    """both directions, every K (under LEVEL each cuts a tie group of an interior node, and the last 30 links are at exactly the
    sensitivity), the all-nodes form and a list with a repeated entry, host and device"""
    nd, params, found = G.lattice3d(medium)
    some = np.array(G.interior()[:5] + G.lattice3d_roots()["corners"] + G.interior()[:1], dtype=np.int32)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in G.DIRS:
            for K in N.KS:
                _neighbours(eng, nd, params, found, d, K, some, "lattice3d %s dir=%d K=%d" % (medium, d, K))
        assert TN._paths(eng) == {"boxes"}
    finally:
        eng.close()


@pytest.mark.parametrize("d", G.DIRS)
def test_lattice3d_hops(rsa, O, d):
    """LEVEL: the four root sets; min_rssi_dbm of -inf, of each shell's exact rssi (the shell stays) and of the next double (it
    goes) -- the walk's level then lies above the sensitivity, except at the last shell, which is the sensitivity itself"""
    nd, params, found = G.lattice3d("LEVEL")
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for label, roots in G.lattice3d_roots().items():
            _hops(eng, nd.n, d, roots, G.hop_tree("LEVEL", d, label), "lattice3d dir=%d roots=%s" % (d, label))
        roots = G.lattice3d_roots()["corner"]
        for k, (r, _) in enumerate(G.shells(found[d], G.interior()[0])):
            for mr in (r, G.up(r)):
                _hops(eng, nd.n, d, roots, G.hop_tree("LEVEL", d, "corner", mr), "lattice3d dir=%d shell %d min=%r" % (d, k, mr), mr, device=k in (0, 7))
        assert TH._paths(eng) == {"boxes"}
    finally:
        eng.close()


@pytest.mark.parametrize("d", G.DIRS)
@pytest.mark.parametrize("kind", ["NONE", "OQPSK"])
def test_lattice3d_routes(rsa, O, kind, d):
    """MARGINAL: the four root sets; every cap of G.CAPS from the corner (128 / 129 decide the 129 shell); min_rssi_dbm at a shell's
    exact rssi and at the next double; host and device forms"""
    nd, params, found = G.lattice3d("MARGINAL")
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for label, roots in G.lattice3d_roots().items():
            what = "lattice3d %s dir=%d roots=%s" % (kind, d, label)
            _routes(eng, nd.n, _p(rsa, kind, d), roots, G.route_tree("MARGINAL", d, label, kind), what)
        roots = G.lattice3d_roots()["corner"]
        for cap in G.CAPS:
            want = G.route_tree("MARGINAL", d, "corner", kind, max_link_cost=cap)
            _routes(eng, nd.n, _p(rsa, kind, d, max_link_cost=cap), roots, want, "lattice3d %s dir=%d cap=%d" % (kind, d, cap), device=cap in (129, 65535))
        sh = G.shells(found[d], G.interior()[0])
        for k in G.ROUTE_SHELLS:
            for mr in (sh[k][0], G.up(sh[k][0])):
                want = G.route_tree("MARGINAL", d, "corner", kind, min_rssi_dbm=mr)
                _routes(eng, nd.n, _p(rsa, kind, d, min_rssi_dbm=mr), roots, want, "lattice3d %s dir=%d shell %d min=%r" % (kind, d, k, mr), device=k == 7)
        assert TR._paths(eng) == {"boxes"}
    finally:
        eng.close()


# ---- 2. wide -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(G.WIDE_L))
def test_wide(rsa, O, path):
    """the probes one double inside and outside the level around a source whose fp32 frame is as coarse as the boxes path trusts
    (slack 0.0475 m), and the same with the frame beyond the limit (the whole-table scan answers): neighbours, hops and routes; and
    the source's HEARD_BY row is a lone tick's result on the same context -- the sweep's own filter at this slack"""
    nd, params, found, who = G.wide(path)
    src = who["src"]
    some = np.array([src] + who["in"][:3] + who["out"][:3] + [0, src], dtype=np.int32)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in G.DIRS:
            _neighbours(eng, nd, params, found, d, 16, some, "wide/%s dir=%d" % (path, d))
            row = eng.neighbors(d, 16, nodes=[src])
            assert row["degree"][0] == G.N_PROBES
            _hops(eng, nd.n, d, [src], H.tree(nd.n, found[d], [src]), "wide/%s dir=%d" % (path, d))
            for kind in ("NONE", "OQPSK"):
                _routes(eng, nd.n, _p(rsa, kind, d), [src], R.tree(nd.n, found[d], [src], G.Q[kind]), "wide/%s %s dir=%d" % (path, kind, d))
        _all_boxes(eng, path)
        assert TN._paths(eng) == TH._paths(eng) == TR._paths(eng) == {path}
        dsrc = DeviceArray(np.array([src], dtype=np.int32))
        try:
            eng.tick_run_sources_device(0, TICK, dsrc.ptr.value, 1, 0, AIR)
            res = eng.result_copy(1, cap=nd.n)
        finally:
            dsrc.free()
        assert res.count == G.N_PROBES and sorted(res.dst.tolist()) == who["in"]
        lone = rsa.Engine.neighbors_from_result(res, 16)
        got = eng.neighbors(N.HEARD_BY, 16, nodes=[src])
        np.testing.assert_array_equal(got["peer"], lone["peer"])
        np.testing.assert_array_equal(_bits(got["rssi"]), _bits(lone["rssi"]))
        assert got["degree"][0] == lone["degree"][0] == res.count
    finally:
        eng.close()


# ---- 3. specials -------------------------------------------------------------------------------------------------------------------

def _check_specials(rsa, eng, nd, params, found, who, what):
    some = np.array(who["power"] + who["rxprob"] + who["off"][:6] + [0], dtype=np.int32)
    roots = [who["power"][1], 0, who["off"][0]]
    for d in G.DIRS:
        _neighbours(eng, nd, params, found, d, 16, some, "%s dir=%d" % (what, d))
        N.same(eng.neighbors(d, 2), N.rows(nd, params, d, 2, None, found[d]), "%s dir=%d K=2" % (what, d))
        _hops(eng, nd.n, d, roots, H.tree(nd.n, found[d], roots), "%s dir=%d" % (what, d))
        for kind, kw in (("NONE", {}), ("OQPSK", {}), ("OQPSK", {"max_link_cost": 431})):
            q = dict(G.Q[kind], **kw)
            _routes(eng, nd.n, _p(rsa, kind, d, **kw), roots, R.tree(nd.n, found[d], roots, q), "%s %s %s dir=%d" % (what, kind, kw, d))


def test_specials(rsa, O):
    """channels that alias in the masks (one negative), 70 radios off over all of them, powers NaN / +inf / -inf / 1e300 and receive
    probabilities NaN / -0.0 / -1.0 / 5e-324: all three queries, both directions, the +inf node and a radio that is off among the
    roots.  Then the four powers back to 0 dBm through rm_node_update (the HEARS cut-off shrinks with the table's new maximum), then
    every power NaN (no node has a power that is a number: all rows empty, only the roots reached)"""
    nd0, params, who = G.specials()
    nd = N._copy(nd0)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        _check_specials(rsa, eng, nd, params, G.specials_links(), who, "specials")
        for j in who["power"]:
            TH._update(eng, nd, j, txpower=0.0)
        _check_specials(rsa, eng, nd, params, G.both(nd, params), who, "specials, powers back to 0")
        for j in range(nd.n):
            TH._update(eng, nd, j, txpower=float("nan"))
        found = G.both(nd, params)
        _check_specials(rsa, eng, nd, params, found, who, "specials, every power NaN")
        for d in G.DIRS:
            got = eng.neighbors(d, 16)
            assert (got["peer"] == -1).all() and (got["degree"] == 0).all() and (_bits(got["rssi"]) == N.NAN_BITS).all()
            assert eng.hops(d, [5, 9])[1] == {"reached": 2, "max_hop": 0, "roots": 2}
            assert eng.routes(_p(rsa, "OQPSK", d), [5, 9])[1] == {"reached": 2, "roots": 2, "max_cost": 0}
        _all_boxes(eng)
    finally:
        eng.close()


# ---- 4. sizes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.SIZES)
def test_sizes(rsa, O, n):
    """65, 1023, 1024 and 1025 nodes of a lattice: all-nodes neighbours with K = 16, hops and routes from node 0, both directions"""
    nd, params, found, _ = G.sizes(n)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in G.DIRS:
            want = N.rows(nd, params, d, 16, None, found[d])
            N.same(eng.neighbors(d, 16), want, "sizes/%d dir=%d host" % (n, d))
            N.same(TN._device_query(eng, d, 16, None, n), want, "sizes/%d dir=%d device" % (n, d))
            _hops(eng, n, d, [0], H.tree(n, found[d], [0]), "sizes/%d dir=%d" % (n, d))
            _routes(eng, n, _p(rsa, "OQPSK", d), [0], R.tree(n, found[d], [0], G.Q["OQPSK"]), "sizes/%d dir=%d" % (n, d))
        _all_boxes(eng)
    finally:
        eng.close()


# ---- 5. many_roots -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", G.DIRS)
def test_many_roots(rsa, O, d):
    """root lists of 16 384, 16 385 and 40 000 entries and every node 23 times over: the seeding kernels' second and third stride
    rounds hold roots that occur nowhere before; the device form also with entries outside the table behind position 16 384"""
    nd, params, found = G.lattice3d("MARGINAL")
    lists, late = G.root_lists()
    eng = _engine(rsa, nd, params)
    try:
        for label, roots in lists.items():
            what = "many_roots/%s dir=%d" % (label, d)
            host = label != "outside"              # (the host forms refuse an entry outside the table)
            want = H.tree(nd.n, found[d], roots)
            assert want["totals"]["roots"] == len(set(roots.tolist()) & set(range(nd.n)))
            _hops(eng, nd.n, d, roots, want, what, host=host)
            _routes(eng, nd.n, _p(rsa, "OQPSK", d), roots, R.tree(nd.n, found[d], roots, G.Q["OQPSK"]), what, host=host)
    finally:
        eng.close()


# ---- 6. hub ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", G.HUB_M)
def test_hub(rsa, O, m):
    """K = 16 against a hub of degree 15, 16 and 17 whose last ten or eleven links tie: the last place is empty, filled, or taken by
    the smaller node index of the tie group, as the rule says; every K, both directions, the boxes path"""
    nd, params, hub = G.hub(m)
    found = G.both(nd, params)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in G.DIRS:
            for K in N.KS:
                _neighbours(eng, nd, params, found, d, K, np.array([hub, 0, hub], dtype=np.int32), "hub/%d dir=%d K=%d" % (m, d, K))
            row = eng.neighbors(d, 16, nodes=[hub])
            assert row["degree"][0] == m and (row["peer"][0] >= 0).sum() == min(m, 16)
        assert TN._paths(eng) == {"boxes"}
    finally:
        eng.close()


# ---- 7. bounds ---------------------------------------------------------------------------------------------------------------------

def test_route_costs_at_their_bounds(rsa, O):
    """a node labelled cost[P] + 129 two rounds before P offers it 128 less one; links of exactly 431 and 1787 that are the only way
    on, under caps on both sides of them"""
    nd, params, found, w = G.bounds()
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in G.DIRS:
            for cap in G.CAPS:
                q = dict(G.Q["OQPSK"], max_link_cost=cap)
                _routes(eng, nd.n, _p(rsa, "OQPSK", d, max_link_cost=cap), [w["R"]], R.tree(nd.n, found[d], [w["R"]], q), "bounds dir=%d cap=%d" % (d, cap))
            got, tot = eng.routes(_p(rsa, "OQPSK", d, max_link_cost=65535), [w["R"]])
            assert [int(got["cost"][w[k]]) for k in "RAPVXY"] == [0, 128, 256, 384, 815, 2602] and tot["reached"] == 6
            _routes(eng, nd.n, _p(rsa, "NONE", d), [w["R"]], R.tree(nd.n, found[d], [w["R"]], G.Q["NONE"]), "bounds NONE dir=%d" % d)
            _hops(eng, nd.n, d, [w["R"]], H.tree(nd.n, found[d], [w["R"]]), "bounds dir=%d" % d)
        _all_boxes(eng)
    finally:
        eng.close()
