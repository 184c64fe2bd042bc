"""The hop query's reference (tests/hops_ref.py) held to the scene conditions the GPU tests rely on, and
the pure host function rm_hops_from_links against it on every scene.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hops_ref as H
import neighbors_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
ALL = H.FIELDS + tuple(H.LINES)


def _root0(name, d, min_rssi=-H.INF):
    nd, _, found = H.scene(name)
    return nd, found[d], H.tree(nd.n, found[d], [0], min_rssi)


def test_n300_levels_and_directions(O):
    """root 0 of n300: deep trees that leave a part of the field out, and the two directions give different trees"""
    want = {d: _root0("n300", d)[2] for d in H.DIRS}
    assert [want[d]["totals"]["max_hop"] for d in H.DIRS] == [17, 26]
    assert [want[d]["totals"]["reached"] for d in H.DIRS] == [174, 193]
    assert (want[H.HEARD_BY]["hop"] != want[H.HEARS]["hop"]).sum() == 116
    assert (want[H.HEARD_BY]["parent"] != want[H.HEARS]["parent"]).sum() == 129
    assert [_root0("n300", d, -85.0)[2]["totals"]["reached"] for d in H.DIRS] == [82, 84]
    assert _root0("n65", H.HEARD_BY)[2]["totals"] == {"reached": 41, "max_hop": 5, "roots": 1}


@pytest.mark.parametrize("name", ["n65", "n300"])
def test_tie_goes_to_the_smaller_index(O, name):
    """unshadowed, roots [A, B]: S is one hop from both on equal rssi bits, and A, the smaller index, is its parent"""
    nd, _, found = H.scene(name)
    sp = N.special(nd)
    for d in H.DIRS:
        w = H.tree(nd.n, found[d], [sp["A"], sp["B"]])
        cand = H.candidates(nd.n, found[d], w)[sp["S"]]
        assert w["hop"][sp["S"]] == 1 and [p for _, p in cand] == [sp["A"], sp["B"]]
        assert N.bits([cand[0][0]])[0] == N.bits([cand[1][0]])[0] == w["rssi"][sp["S"]]
        assert w["parent"][sp["S"]] == sp["A"] < sp["B"]


@pytest.mark.parametrize("name", N.RICH)
def test_parent_choice_is_not_trivial(O, name):
    """every rich scene, root 0: the parent is neither simply the node's strongest link nor simply the first candidate found"""
    for d in H.DIRS:
        nd, found, w = _root0(name, d)
        cand = H.candidates(nd.n, found, w)
        strongest = {j: sorted(found[j], key=lambda f: (-f[0], f[1]))[0][1] for j in cand}
        assert sum(1 for j in cand if w["parent"][j] != strongest[j]) >= 35
        assert sum(1 for j in cand if w["parent"][j] != min(p for _, p in cand[j])) >= 10
        assert sum(1 for j in cand if len(cand[j]) > 1) >= 15
        assert w["children"].sum() == w["totals"]["reached"] - 1 and w["children"].max() > 1


@pytest.mark.parametrize("name", N.RICH + tuple(H.BIG))
def test_the_lone_node_reaches_only_itself(O, name):
    nd, _, found = H.scene(name)
    lone = N.special(nd)["LONE"]
    for d in H.DIRS:
        w = H.tree(nd.n, found[d], [lone])
        assert w["totals"] == {"reached": 1, "max_hop": 0, "roots": 1} and w["hop"][lone] == 0 and (np.delete(w["hop"], lone) == -1).all()


@pytest.mark.parametrize("name, n", [("line40", 40), ("line70", 70)])
def test_lines(O, name, n):
    """one node per level"""
    for d in H.DIRS:
        nd, _, w = _root0(name, d)
        assert w["totals"] == {"reached": n, "max_hop": n - 1, "roots": 1}
        np.testing.assert_array_equal(w["hop"], np.arange(n))
        np.testing.assert_array_equal(w["parent"], np.arange(n) - 1)


def test_n3000(O):
    """rich(3000, 5), root 0: nearly the whole field, tens of levels, and a level that spans several workgroups of frontier waves"""
    got = [_root0("n3000_shadow", d)[2] for d in H.DIRS]
    assert [w["totals"]["reached"] for w in got] == [2879, 2978]
    assert [w["totals"]["max_hop"] for w in got] == [33, 35]
    assert [int(np.bincount(w["hop"][w["hop"] >= 0]).max()) for w in got] == [365, 363]


# ---- rm_hops_from_links against the reference --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_from_links_against_the_reference(rsa, O, name):
    """every scene, both directions, min_rssi_dbm -inf and -85, the tests' root sets, every optional output left out in turn"""
    nd, _, found = H.scene(name)
    for d in H.DIRS:
        node, far, rssi = H.flat(found[d])
        order = np.random.default_rng(3).permutation(len(node))   # (the answer does not depend on the list's order)
        for label, roots in H.root_sets(nd, name).items():
            if nd.n > 1000 and label not in ("0", "A,B", "all"):
                continue
            for mr in (-H.INF, -85.0):
                what = "%s dir=%d roots=%s min=%s" % (name, d, label, mr)
                want = H.tree(nd.n, found[d], roots, mr)
                got, tot = rsa.Engine.hops_from_links(nd.n, node[order], far[order], rssi[order], roots, mr)
                H.same(got, tot, want, what)
        want = H.tree(nd.n, found[d], [0])
        for fields in ((), ("parent",), ("rssi",), ("children",)):
            got, tot = rsa.Engine.hops_from_links(nd.n, node, far, rssi, [0], fields=fields)
            assert set(got) == {"hop"} | set(fields)
            H.same(got, tot, want, "%s dir=%d fields=%s" % (name, d, fields))


def test_from_links_entries_that_are_no_links(rsa):
    """a NaN rssi, node == far, rssi below min_rssi_dbm; rssi == min_rssi_dbm is a link; +inf keeps none; two entries of one pair"""
    node = np.array([1, 1, 2, 2, 3, 3, 3], dtype=np.int32)
    far = np.array([0, 1, 1, 0, 2, 1, 1], dtype=np.int32)
    rssi = np.array([-70.0, -10.0, -80.0, float("nan"), -90.0, -95.0, -60.0])
    got, tot = rsa.Engine.hops_from_links(5, node, far, rssi, [0])
    assert got["hop"].tolist() == [0, 1, 2, 2, -1] and got["parent"].tolist() == [-1, 0, 1, 1, -1] and got["children"].tolist() == [1, 2, 0, 0, 0]
    assert N.bits(got["rssi"]).tolist() == [N.NAN_BITS] + N.bits([-70.0, -80.0, -60.0]).tolist() + [N.NAN_BITS]
    assert tot == {"reached": 4, "max_hop": 2, "roots": 1}
    assert rsa.Engine.hops_from_links(5, node, far, rssi, [0], -80.0)[1] == {"reached": 4, "max_hop": 2, "roots": 1}
    assert rsa.Engine.hops_from_links(5, node, far, rssi, [0], np.nextafter(-80.0, 0.0))[0]["hop"].tolist() == [0, 1, -1, 2, -1]
    assert rsa.Engine.hops_from_links(5, node, far, rssi, [0, 4, 0], H.INF)[1] == {"reached": 2, "max_hop": 0, "roots": 2}
    assert rsa.Engine.hops_from_links(5, node, far, rssi, [])[1] == {"reached": 0, "max_hop": -1, "roots": 0}
    assert rsa.Engine.hops_from_links(0, [], [], [], [])[1] == {"reached": 0, "max_hop": -1, "roots": 0}


def test_from_links_under_sanitizers(rsa, tmp_path):
    """tests/cpp/hops_host_san_test.cpp with rm_api_hops.cpp compiled beside it under -fsanitize=address,undefined (host code only:
    the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "hops_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_hops.cpp"), os.path.join(ROOT, "tests", "cpp", "hops_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)


def test_from_links_refusals(rsa):
    L = rsa._lib.lib()
    hop = np.zeros(4, dtype=np.int32)
    st = rsa.HopsOut(hop=hop.ctypes.data)
    one = np.array([1], dtype=np.int32)
    r = np.array([-50.0])
    import ctypes as C

    def call(n_nodes, n_links, node, far, rssi, mr, roots, n_roots, out):
        return L.rm_hops_from_links(n_nodes, n_links, node, far, rssi, mr, roots, n_roots, out, None)

    ok = (4, 1, one.ctypes.data, one.ctypes.data, r.ctypes.data, -90.0, one.ctypes.data, 1, C.byref(st))
    assert call(*ok) == 0
    for k, v in ((8, None), (8, C.byref(rsa.HopsOut())), (5, float("nan")), (0, -1), (1, -1), (7, -1), (2, None), (3, None), (4, None), (6, None)):
        bad = list(ok)
        bad[k] = v
        assert call(*bad) == INVALID, (k, v)
    for roots in ([4], [-1]):
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.hops_from_links(4, [1], [0], [-50.0], roots)
        assert e.value.code == INVALID
    for node, far in (([4], [0]), ([0], [4]), ([-1], [0]), ([0], [-2 ** 31])):
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.hops_from_links(4, node, far, [-50.0], [0])
        assert e.value.code == INVALID
