"""Reference of the hop query.  It stands on tests/neighbors_ref.py::links -- the oracle's potential
links -- alone: a level-by-level breadth-first search in plain Python over those links, the parent chosen by the rule (rssi
descending, ties by the smaller node index) among the links one level closer.  No engine code is involved and the library's exports
are never the source of an expected value.  tests/test_hops_ref.py holds the scenes' conditions for this reference alone, so that no
GPU test passes vacuously."""
import numpy as np

from oracle import oracle as O

import neighbors_ref as N

HEARD_BY, HEARS = N.HEARD_BY, N.HEARS
DIRS = (HEARD_BY, HEARS)
NAN_BITS = N.NAN_BITS
INF = float("inf")


def line(n):
    """n nodes in a row, 60 m apart, txpower 0: under PLAIN the reach is 68 m, node i's only links are i - 1 and i + 1"""
    nd = O.NodeTable(n)
    nd.x = 60.0 * np.arange(n)
    nd.txpower = np.zeros(n)
    return nd


LINES = {"line40": (lambda: line(40), N.PLAIN), "line70": (lambda: line(70), N.PLAIN)}
BIG = {"n3000_shadow": (lambda: N.rich(3000, 5), N.SHADOW)}   # three boxes of 1024 receivers
FIELDS = tuple(N.SCENES) + tuple(BIG)
_CACHE = {}


def scene(name):
    """-> (nd, params, {direction: links of all nodes}); computed once, shared and left unchanged"""
    if name in N.SCENES:
        return N.scene(name)
    if name not in _CACHE:
        make, params = {**LINES, **BIG}[name]
        nd = make()
        _CACHE[name] = (nd, params, {d: N.links(nd, params, d) for d in DIRS})
    return _CACHE[name]


def tree(n, found, roots, min_rssi=-INF):
    """the rule over the links of one direction ({node: [(rssi, far end)]}: the far end may be the node's parent) ->
    {"hop", "parent", "rssi" (bits), "children", "totals"}; a root outside the table is ignored"""
    hop = np.full(n, -1, dtype=np.int32)
    parent = np.full(n, -1, dtype=np.int32)
    rb = np.full(n, NAN_BITS, dtype=np.uint64)
    children = np.zeros(n, dtype=np.int32)
    keep = {j: [(r, p) for r, p in found.get(j, ()) if r == r and r >= min_rssi and p != j] for j in range(n)}
    below = {p: [] for p in range(n)}   # the nodes a node may be the parent of
    for j, ls in keep.items():
        for _, p in ls:
            below[p].append(j)
    frontier = []
    for r in [int(r) for r in np.asarray(roots).reshape(-1).tolist()]:
        if 0 <= r < n and hop[r] == -1:
            hop[r] = 0
            frontier.append(r)
    n_roots, level, reached, max_hop = len(frontier), 0, 0, -1
    while frontier:
        max_hop = level
        reached += len(frontier)
        nxt = []
        for p in frontier:
            for j in below[p]:
                if hop[j] == -1:
                    hop[j] = level + 1
                    nxt.append(j)
        frontier, level = nxt, level + 1
    for j in range(n):
        if hop[j] >= 1:
            cand = sorted([(-r, p) for r, p in keep[j] if hop[p] == hop[j] - 1])
            parent[j] = cand[0][1]
            rb[j] = N.bits([-cand[0][0]])[0]
            children[parent[j]] += 1
    return {"hop": hop, "parent": parent, "rssi": rb, "children": children,
            "totals": {"reached": reached, "max_hop": max_hop, "roots": n_roots}}


def candidates(n, found, want, min_rssi=-INF):
    """per reached non-root node, its parent candidates [(rssi, far end)] in the rule's order"""
    hop = want["hop"]
    return {j: sorted([(r, p) for r, p in found[j] if r == r and r >= min_rssi and hop[p] == hop[j] - 1], key=lambda f: (-f[0], f[1]))
            for j in range(n) if hop[j] >= 1}


def same(got, totals, want, what):
    """exact equality of a query's outputs ({"hop", ...}; parent / rssi / children may be missing) and totals with tree()"""
    np.testing.assert_array_equal(got["hop"], want["hop"], err_msg=what + ": hop")
    if "parent" in got:
        np.testing.assert_array_equal(got["parent"], want["parent"], err_msg=what + ": parent")
    if "rssi" in got:
        np.testing.assert_array_equal(N.bits(got["rssi"]), want["rssi"], err_msg=what + ": rssi bits")
    if "children" in got:
        np.testing.assert_array_equal(got["children"], want["children"], err_msg=what + ": children")
    if totals is not None:
        assert totals == want["totals"], (what, totals, want["totals"])


def flat(found):
    """the links of one direction as the three columns rm_hops_from_links takes"""
    node = [j for j, ls in found.items() for _ in ls]
    far = [p for ls in found.values() for _, p in ls]
    rssi = [r for ls in found.values() for r, _ in ls]
    return np.array(node, dtype=np.int32), np.array(far, dtype=np.int32), np.array(rssi, dtype=np.float64)


def root_sets(nd, name):
    """the root sets of the tests -> {label: roots}"""
    n = nd.n
    sets = {"0": [0], "all": list(range(n)), "none": [], "dup": [0, n - 1, 0, 0, n - 1]}
    if name in N.RICH or name in BIG:
        sp = N.special(nd)
        sets.update({"0,S": [0, sp["S"]], "A,B": [sp["A"], sp["B"]], "LOUD": [sp["LOUD"]], "LONE": [sp["LONE"]]})
    return sets
