"""The route query's reference (tests/routes_ref.py) held to the scene conditions the GPU tests rely on,
and the pure host functions rm_routes_link_cost and rm_routes_from_links against it on every scene.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hops_ref as H
import neighbors_ref as N
import routes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
ALL = H.FIELDS + tuple(R.LADDERS)
Q = {k: v[0] for k, v in R.SETS.items()}


def _params(rsa, q, direction=0, **kw):
    return rsa.Engine.routes_params(direction=direction, **dict(q, **kw))


def test_marginal_scene_is_not_the_hop_tree(O):
    """MARGINAL on n300_shadow, root 0, both directions: many links cost more than 128, many are over the cap, many nodes have
    another parent than the hop query's, sit deeper than their hop count, or choose among several equal-cost candidates
    (measured: 2 018 within the cap, 1 415 over it, 121 / 143, 100 / 94, 62 / 71)"""
    q = Q["MARGINAL"]
    nd, _, found = R.scene("n300_shadow", "MARGINAL")
    for d in R.DIRS:
        costs = [R.link_cost(q, r) for j in range(nd.n) for r, _ in found[d][j]]
        assert sum(1 for c in costs if c is not None and c > 128) >= 1000
        assert sum(1 for c in costs if c is None) >= 500
        w, h = R.tree(nd.n, found[d], [0], q), H.tree(nd.n, found[d], [0])
        assert ((w["parent"] != h["parent"]) & (w["cost"] != R.UNREACHED)).sum() >= 50
        dep = R.depth(w)
        assert ((dep > h["hop"]) & (dep >= 0)).sum() >= 50
        cand = R.candidates(nd.n, found[d], w, q)
        assert sum(1 for j in cand if len(cand[j]) > 1) >= 20
        assert w["children"].sum() == w["totals"]["reached"] - 1
        assert (w["cost"][w["parent"] >= 0] == w["cost"][w["parent"][w["parent"] >= 0]] + w["link_cost"][w["parent"] >= 0]).all()


def test_the_cap_leaves_nodes_out(O):
    """n300 without shadowing, HEARD_BY: a node the hop query reaches and the route query does not"""
    nd, _, found = R.scene("n300", "MARGINAL")
    w, h = R.tree(nd.n, found[R.HEARD_BY], [0], Q["MARGINAL"]), H.tree(nd.n, found[R.HEARD_BY], [0])
    assert ((h["hop"] >= 0) & (w["cost"] == R.UNREACHED)).sum() >= 1
    assert not ((h["hop"] < 0) & (w["cost"] != R.UNREACHED)).any()


@pytest.mark.parametrize("name", H.FIELDS)
def test_defaults_give_the_hop_tree(O, name):
    """OQPSK at the model's defaults: every potential link has an SNR of 5 dB and more, every cost is 128, the tree is the hop query's;
    and NONE gives it by construction"""
    nd, _, found = R.scene(name, "OQPSK")
    for d in R.DIRS:
        assert all(R.link_cost(Q["OQPSK"], r) == 128 for j in range(nd.n) for r, _ in found[d][j])
        for roots in ([0], [0, nd.n - 1]):
            h = H.tree(nd.n, found[d], roots)
            for pset in ("OQPSK", "NONE"):
                w = R.tree(nd.n, found[d], roots, Q[pset])
                np.testing.assert_array_equal(w["cost"], np.where(h["hop"] >= 0, 128 * h["hop"].astype(np.int64), -1).astype(np.uint64))
                for f in ("parent", "rssi", "children"):
                    np.testing.assert_array_equal(w[f], h[f])
                assert w["totals"] == {"reached": h["totals"]["reached"], "roots": h["totals"]["roots"], "max_cost": 128 * max(h["totals"]["max_hop"], 0)}


@pytest.mark.parametrize("name, n", [("ladder40", 40), ("ladder70", 70)])
def test_ladders(O, name, n):
    """rows 55 m apart under MARGINAL: the two-step link costs more than twice the one-step link, so the routes follow the chain
    while the hops skip -- a relaxation labels every node too high first and lowers it later"""
    q = Q["MARGINAL"]
    nd, _, found = R.scene(name, "MARGINAL")
    for d in R.DIRS:
        one = {R.link_cost(q, r) for r, p in found[d][5] if abs(p - 5) == 1}
        two = {R.link_cost(q, r) for r, p in found[d][5] if abs(p - 5) == 2}
        assert len(found[d][5]) == 4 and one == {128} and len(two) == 1 and min(two) > 2 * 128
        w, h = R.tree(nd.n, found[d], [0], q), H.tree(nd.n, found[d], [0])
        np.testing.assert_array_equal(w["parent"], np.arange(n) - 1)
        np.testing.assert_array_equal(w["cost"], 128 * np.arange(n, dtype=np.uint64))
        assert h["totals"]["max_hop"] == n // 2 and w["totals"] == {"reached": n, "roots": 1, "max_cost": 128 * (n - 1)}


# ---- rm_routes_link_cost ------------------------------------------------------------------------------------------------------

def test_link_cost_known_answers(rsa, O):
    cost = rsa.Engine.route_link_cost
    none, oq = _params(rsa, Q["NONE"]), _params(rsa, Q["OQPSK"])
    assert cost(none, -100.0, -94.0) == 128 and cost(none, -100.0, -300.0) == 128 and cost(oq, -100.0, -60.0) == 128
    assert cost(oq, -100.0, -R.INF) is None and cost(oq, -100.0, float("nan")) is None
    assert cost(_params(rsa, Q["NONE"], min_rssi_dbm=-90.0), -100.0, -R.INF) is None
    for q in (Q["NONE"], Q["OQPSK"]):
        assert cost(_params(rsa, q, min_rssi_dbm=-90.0), -100.0, -90.0) == 128
        assert cost(_params(rsa, q, min_rssi_dbm=-90.0), -100.0, float(np.nextafter(-90.0, -R.INF))) is None
        assert cost(_params(rsa, q, min_rssi_dbm=R.INF), -100.0, -60.0) is None
    # the cap boundary: a link whose cost is exactly the cap counts, one above it does not; the smallest and the largest cap
    r = -101.0
    c = R.link_cost(dict(Q["OQPSK"], max_link_cost=65535), r)
    assert 128 < c < 65535
    assert cost(_params(rsa, Q["OQPSK"], max_link_cost=c), -100.0, r) == c
    assert cost(_params(rsa, Q["OQPSK"], max_link_cost=c - 1), -100.0, r) is None
    assert cost(_params(rsa, Q["OQPSK"], max_link_cost=128), -100.0, r) is None and cost(_params(rsa, Q["OQPSK"], max_link_cost=128), -100.0, -60.0) == 128
    # a sweep through the transition, other air times, bit times and noise floors, against the reference
    for q, noise in ((Q["MARGINAL"], -100.0), (dict(Q["OQPSK"], air_us=640, max_link_cost=65535), -100.0), (dict(Q["OQPSK"], us_per_bit=2.0), -97.3),
                     (dict(Q["OQPSK"], air_us=0), -100.0)):
        seen = set()
        for r in np.arange(-106.0, -92.0, 1.0 / 64).tolist() + [-80.0, 0.0, 40.0, R.INF]:
            want = R.link_cost(q, r, noise)
            assert cost(_params(rsa, q), noise, r) == want, (q, noise, r)
            seen.add(want)
        # (not vacuous: the sweep crosses the transition -- costs of 128, many between, and links over the cap)
        assert (len(seen) >= 20 and {None, 128} <= seen) or (q["air_us"] == 0 and seen == {128})


def test_the_array_form_of_the_reference_is_the_scalar_form(O):
    """routes_ref.link_costs_np (numpy, for the 65 537-node certificate) equals routes_ref.link_cost (the oracle's orc_det_*) on a
    sweep through the transition, its ends, and every link rssi of the marginal scene"""
    _, _, found = R.scene("n300_shadow", "MARGINAL")
    rssi = np.array(np.arange(-106.0, -92.0, 1.0 / 64).tolist() + [-300.0, -80.0, 0.0, 40.0, R.INF, -R.INF, float("nan")]
                    + [r for ls in found[R.HEARD_BY].values() for r, _ in ls])
    for q in (Q["NONE"], Q["MARGINAL"], dict(Q["OQPSK"], air_us=640, max_link_cost=65535, min_rssi_dbm=-101.0), dict(Q["OQPSK"], air_us=0, us_per_bit=2.0)):
        want = [R.link_cost(q, r) for r in rssi.tolist()]
        np.testing.assert_array_equal(R.link_costs_np(q, rssi), np.array([-1 if c is None else c for c in want], dtype=np.int64))
        assert None in want and 128 in want


def test_link_cost_refusals(rsa):
    bad = ({"kind": 2}, {"kind": -1}, {"reserved": 1}, {"us_per_bit": 0.0}, {"us_per_bit": -4.0}, {"us_per_bit": R.INF}, {"us_per_bit": float("nan")},
           {"air_us": -1}, {"min_rssi_dbm": float("nan")}, {"max_link_cost": 127}, {"max_link_cost": 65536})
    for kw in bad:
        assert rsa.Engine.route_link_cost(_params(rsa, Q["OQPSK"], **kw), -100.0, -60.0) is None, kw
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.routes_from_links(2, [1], [0], [-60.0], _params(rsa, Q["OQPSK"], **kw), -100.0, [0])
        assert e.value.code == INVALID, kw
    assert rsa.Engine.route_link_cost(_params(rsa, Q["OQPSK"], direction=7), -100.0, -60.0) == 128   # (direction is not looked at)


# ---- rm_routes_from_links against the reference -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_from_links_against_the_reference(rsa, O, name):
    """every scene, both directions, the three parameter sets, the tests' root sets, min_rssi_dbm and another cap, every optional
    output left out in turn"""
    for pset in R.SETS:
        if name in R.LADDERS and pset != "MARGINAL":
            continue
        nd, _, found = R.scene(name, pset)
        for d in R.DIRS:
            node, far, rssi = H.flat(found[d])
            order = np.random.default_rng(3).permutation(len(node))   # (the answer does not depend on the list's order)
            for label, roots in H.root_sets(nd, name).items():
                if nd.n > 1000 and label not in ("0", "A,B"):
                    continue
                for kw in ({}, {"min_rssi_dbm": -85.0}, {"max_link_cost": 300}) if label in ("0", "0,S", "all") and nd.n <= 1000 else ({},):
                    q = dict(Q[pset], **kw)
                    what = "%s %s dir=%d roots=%s %s" % (name, pset, d, label, kw)
                    got, tot = rsa.Engine.routes_from_links(nd.n, node[order], far[order], rssi[order], _params(rsa, q), R.NOISE_DBM, roots)
                    R.same(got, tot, R.tree(nd.n, found[d], roots, q), what)
            want = R.tree(nd.n, found[d], [0], Q[pset])
            for fields in ((), ("parent",), ("rssi",), ("link_cost",), ("children",)):
                got, tot = rsa.Engine.routes_from_links(nd.n, node, far, rssi, _params(rsa, Q[pset]), R.NOISE_DBM, [0], fields=fields)
                assert set(got) == {"cost"} | set(fields)
                R.same(got, tot, want, "%s %s dir=%d fields=%s" % (name, pset, d, fields))


def test_from_links_entries_that_are_no_links(rsa, O):
    """a NaN rssi, node == far, rssi below min_rssi_dbm, a link over the cap; two entries of one pair; duplicated roots"""
    q = dict(Q["MARGINAL"], min_rssi_dbm=-102.0)
    node = np.array([1, 1, 2, 2, 3, 3, 3, 2], dtype=np.int32)
    far = np.array([0, 1, 1, 0, 2, 1, 1, 0], dtype=np.int32)
    rssi = np.array([-70.0, -10.0, -101.0, float("nan"), -90.0, -102.5, -60.0, -102.0])
    c101, c102 = R.link_cost(q, -101.0), R.link_cost(q, -102.0)
    assert 128 < c101 < 1024 and c102 is None and R.link_cost(Q["MARGINAL"], -102.5) is None
    got, tot = rsa.Engine.routes_from_links(5, node, far, rssi, _params(rsa, q), R.NOISE_DBM, [0, 0])
    assert got["cost"].tolist() == [0, 128, 128 + c101, 256, R.UNREACHED] and got["parent"].tolist() == [-1, 0, 1, 1, -1]
    assert got["link_cost"].tolist() == [0, 128, c101, 128, 0] and got["children"].tolist() == [1, 2, 0, 0, 0]
    assert N.bits(got["rssi"]).tolist() == [N.NAN_BITS] + N.bits([-70.0, -101.0, -60.0]).tolist() + [N.NAN_BITS]
    assert tot == {"reached": 4, "roots": 1, "max_cost": 128 + c101}
    R.same(got, tot, R.tree(5, {1: [(-70.0, 0), (-10.0, 1)], 2: [(-101.0, 1), (float("nan"), 0), (-102.0, 0)], 3: [(-90.0, 2), (-102.5, 1), (-60.0, 1)]},
                            [0, 0], q), "the reference agrees")
    assert rsa.Engine.routes_from_links(5, node, far, rssi, _params(rsa, q), R.NOISE_DBM, [])[1] == {"reached": 0, "roots": 0, "max_cost": 0}
    assert rsa.Engine.routes_from_links(0, [], [], [], _params(rsa, q), R.NOISE_DBM, [])[1] == {"reached": 0, "roots": 0, "max_cost": 0}


def test_from_links_under_sanitizers(rsa, tmp_path):
    """tests/cpp/routes_host_san_test.cpp with rm_api_routes.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "routes_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_routes.cpp"), os.path.join(ROOT, "tests", "cpp", "routes_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)


def test_from_links_refusals(rsa):
    import ctypes as C
    L = rsa._lib.lib()
    cost = np.zeros(4, dtype=np.uint64)
    st = rsa.RoutesOut(cost=cost.ctypes.data)
    one = np.array([1], dtype=np.int32)
    r = np.array([-50.0])
    prm = _params(rsa, Q["OQPSK"])

    def call(n_nodes, n_links, node, far, rssi, params, noise, roots, n_roots, out):
        return L.rm_routes_from_links(n_nodes, n_links, node, far, rssi, params, noise, roots, n_roots, out, None)

    ok = (4, 1, one.ctypes.data, one.ctypes.data, r.ctypes.data, C.byref(prm), -100.0, one.ctypes.data, 1, C.byref(st))
    assert call(*ok) == 0
    for k, v in ((9, None), (9, C.byref(rsa.RoutesOut())), (5, None), (0, -1), (1, -1), (8, -1), (2, None), (3, None), (4, None), (7, None)):
        bad = list(ok)
        bad[k] = v
        assert call(*bad) == INVALID, (k, v)
    for roots in ([4], [-1]):
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.routes_from_links(4, [1], [0], [-50.0], prm, -100.0, roots)
        assert e.value.code == INVALID
    for node, far in (([4], [0]), ([0], [4]), ([-1], [0]), ([0], [-2 ** 31])):
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.routes_from_links(4, node, far, [-50.0], prm, -100.0, [0])
        assert e.value.code == INVALID
