"""Reference of the route query.  It stands on tests/neighbors_ref.py::links -- the oracle's potential
links -- and tests/errmodel_ref.py::psr alone, with the oracle's orc_det_* for the SNR: a link's cost written from the spec with
Python's IEEE doubles (one rounding per operation, no fma), a plain-Python Dijkstra over the counting links, and the parent chosen by
the rule (rssi descending, ties by the smaller node index) among the links on a least-cost path.  No engine code is involved and
the library's exports are never the source of an expected value.  tests/test_routes_ref.py holds the scenes' conditions for this
reference alone, so that no GPU test passes vacuously."""
import heapq
import math

import numpy as np

from oracle import oracle as O

import errmodel_ref as EM
import hops_ref as H
import neighbors_ref as N

HEARD_BY, HEARS, DIRS = H.HEARD_BY, H.HEARS, H.DIRS
NAN_BITS = N.NAN_BITS
INF = float("inf")
UNREACHED = 0xFFFFFFFFFFFFFFFF
EM_NONE, EM_OQPSK = 0, 1
NOISE_DBM = -100.0   # the oracle's default noise floor; no scene changes it
FIELDS = ("cost", "parent", "rssi", "link_cost", "children")

# the parameter sets: (the query's parameters, what the set changes in a scene's model)
_Q = {"us_per_bit": 4.0, "air_us": 4064, "min_rssi_dbm": -INF, "max_link_cost": 1024}
SETS = {
    "NONE": (dict(_Q, kind=EM_NONE), {}),
    "OQPSK": (dict(_Q, kind=EM_OQPSK), {}),
    "MARGINAL": (dict(_Q, kind=EM_OQPSK), {"ld_sensitivity_dbm": -103.0}),
}


def noise_db(noise_dbm=NOISE_DBM):
    """10 * det_log10(ld_noise_lin), ld_noise_lin = det_pow10(noise / 10) as the model derives it"""
    L = O.lib()
    return 10.0 * L.orc_det_log10(L.orc_det_pow10(noise_dbm / 10.0))


_COST = {}


def link_cost(q, rssi, noise_dbm=NOISE_DBM):
    """the rule's link cost from the link's rssi -> an int in 128 .. max_link_cost, or None when the link does not count"""
    rssi = float(rssi)
    if not rssi >= q["min_rssi_dbm"]:
        return None
    key = (q["kind"], q["us_per_bit"], q["air_us"], q["max_link_cost"], noise_dbm, rssi.hex())
    if key not in _COST:
        snr = rssi - noise_db(noise_dbm)
        psr = 1.0 if q["kind"] == EM_NONE else EM.psr(snr, q["air_us"], q["us_per_bit"])
        c = None
        if psr > 0.0:
            v = 128.0 / psr
            v = math.floor(v + 0.5) if v == v and v != INF else v
            if v <= float(q["max_link_cost"]):
                c = int(v)
        _COST[key] = c
    return _COST[key]


# ---- the same cost over an array, for the tables the scalar form is too slow for: the spec's operations in numpy's IEEE doubles (one
# rounding per ufunc, no fma), written from the spec's text of det_log2 / det_exp2; tests/test_routes_ref.py holds it to link_cost

def _np_log2(x):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    e = ((b >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    m = ((b & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    f = (m - 1.0) / (m + 1.0)
    s = f * f
    q = np.full_like(f, 1.0 / 23.0)
    for k in range(10, 0, -1):
        q = q * s + 1.0 / float(2 * k + 1)
    q = q * s
    r = f + f * q
    return e.astype(np.float64) + (2.0 * r) * 1.4426950408889634


def _np_exp2(y):
    y = np.asarray(y, dtype=np.float64)
    inside = (y >= -1022.0) & (y <= 1023.0)
    yy = np.where(inside, y, 0.0)
    k = np.floor(yy + 0.5)
    t = (yy - k) * 0.6931471805599453
    q = np.full_like(t, 1.0 / float(math.factorial(13)))
    for n in range(12, -1, -1):
        q = q * t + 1.0 / float(math.factorial(n))
    scale = ((k.astype(np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    out = q * scale
    out = np.where(y > 1023.0, INF, np.where(y >= -1022.0, out, 0.0))
    return np.where(y != y, y, out)


def link_costs_np(q, rssi, noise_dbm=NOISE_DBM):
    """link_cost over an array of finite or infinite rssi values -> int64, -1 where the link does not count"""
    rssi = np.asarray(rssi, dtype=np.float64)
    with np.errstate(all="ignore"):
        if q["kind"] == EM_NONE:
            psr = np.ones_like(rssi)
        else:
            snr = rssi - noise_db(noise_dbm)
            s = _np_exp2((snr / 10.0) * 3.3219280948873622)
            acc = np.zeros_like(s)
            for k in range(2, 17):
                ck = 1.0 / float(k) - 1.0
                tk = EM.BINOM[k] * _np_exp2(((20.0 * s) * ck) * 1.4426950408889634)
                acc = acc + tk if k % 2 == 0 else acc - tk
            b = acc / 30.0
            b = np.where(b < 0.0, 0.0, b)
            b = np.where(0.5 < b, 0.5, b)
            psr = _np_exp2((float(int(q["air_us"])) / q["us_per_bit"]) * _np_log2(1.0 - b))
            psr = np.where(b != b, b, psr)
        c = np.floor(128.0 / psr + 0.5)
        ok = (rssi >= q["min_rssi_dbm"]) & (psr > 0.0) & (c <= float(q["max_link_cost"]))
        return np.where(ok, np.where(ok, c, 0.0).astype(np.int64), -1)


def ladder(n, step=55.0):
    """n nodes in a row, `step` m apart, txpower 0 (hops_ref.line with another spacing)"""
    nd = O.NodeTable(n)
    nd.x = step * np.arange(n)
    nd.txpower = np.zeros(n)
    return nd


LADDERS = {"ladder40": (lambda: ladder(40), N.PLAIN), "ladder70": (lambda: ladder(70), N.PLAIN)}
_CACHE = {}


def scene(name, pset):
    """-> (nd, the scene's model parameters under the set, {direction: links of all nodes}); computed once, shared, left unchanged"""
    over = SETS[pset][1]
    if not over and name not in LADDERS:
        return H.scene(name)
    if (name, pset) not in _CACHE:
        if name in LADDERS:
            make, base = LADDERS[name]
            nd = make()
        else:
            nd, base, _ = H.scene(name)
        params = dict(base, **over)
        _CACHE[(name, pset)] = (nd, params, {d: N.links(nd, params, d) for d in DIRS})
    return _CACHE[(name, pset)]


def counting(n, found, q):
    """{node: [(rssi, far end, cost)]} of the counting links.  A table of more than 1000 nodes takes the array form of the cost
    (link_costs_np, held to link_cost by tests/test_routes_ref.py): the scalar form would take tens of seconds there."""
    out = {}
    if n > 1000:
        flat = [(j, r, p) for j in range(n) for r, p in found.get(j, ()) if p != j and r == r]
        costs = link_costs_np(q, np.array([r for _, r, _ in flat], dtype=np.float64)).tolist() if flat else []
        out = {j: [] for j in range(n)}
        for (j, r, p), c in zip(flat, costs):
            if c >= 0:
                out[j].append((r, p, c))
        return out
    for j in range(n):
        ls = []
        for r, p in found.get(j, ()):
            if p != j and r == r:
                c = link_cost(q, r)
                if c is not None:
                    ls.append((r, p, c))
        out[j] = ls
    return out


def tree(n, found, roots, q):
    """the rule over the links of one direction ({node: [(rssi, far end)]}: the far end may be the node's parent) ->
    {"cost", "parent", "rssi" (bits), "link_cost", "children", "totals"}; a root outside the table is ignored"""
    keep = counting(n, found, q)
    below = {p: [] for p in range(n)}   # the nodes a node may be the parent of, with the link's cost
    for j, ls in keep.items():
        for _, p, c in ls:
            below[p].append((j, c))
    cost = [None] * n
    heap = []
    for r in [int(r) for r in np.asarray(roots).reshape(-1).tolist()]:
        if 0 <= r < n and cost[r] is None:
            cost[r] = 0
            heap.append((0, r))
    n_roots = len(heap)
    heapq.heapify(heap)
    done = [False] * n
    while heap:
        cp, p = heapq.heappop(heap)
        if done[p]:
            continue
        done[p] = True
        for j, c in below[p]:
            if cost[j] is None or cp + c < cost[j]:
                cost[j] = cp + c
                heapq.heappush(heap, (cp + c, j))
    parent = np.full(n, -1, dtype=np.int32)
    rb = np.full(n, NAN_BITS, dtype=np.uint64)
    lc = np.zeros(n, dtype=np.uint32)
    children = np.zeros(n, dtype=np.int32)
    for j in range(n):
        if cost[j]:
            cand = sorted([(-r, p, c) for r, p, c in keep[j] if cost[p] is not None and cost[p] + c == cost[j]])
            parent[j], lc[j] = cand[0][1], cand[0][2]
            rb[j] = N.bits([-cand[0][0]])[0]
            children[parent[j]] += 1
    reached = [c for c in cost if c is not None]
    return {"cost": np.array([UNREACHED if c is None else c for c in cost], dtype=np.uint64), "parent": parent, "rssi": rb, "link_cost": lc,
            "children": children, "totals": {"reached": len(reached), "roots": n_roots, "max_cost": max(reached, default=0)}}


def candidates(n, found, want, q):
    """per reached non-root node, its parent candidates [(rssi, far end, cost)] in the rule's order"""
    keep = counting(n, found, q)
    cost = want["cost"].tolist()
    return {j: sorted([(r, p, c) for r, p, c in keep[j] if cost[p] != UNREACHED and cost[p] + c == cost[j]], key=lambda f: (-f[0], f[1]))
            for j in range(n) if cost[j] not in (0, UNREACHED)}


def depth(want):
    """the hop count along the chosen routes (-1: not reached)"""
    parent, cost = want["parent"], want["cost"]
    d = np.full(len(parent), -1, dtype=np.int64)
    d[cost == 0] = 0
    for j in np.argsort(cost, kind="stable").tolist():
        if parent[j] >= 0:
            d[j] = d[parent[j]] + 1
    return d


def same(got, totals, want, what):
    """exact equality of a query's outputs ({"cost", ...}; the others may be missing) and totals with tree()"""
    np.testing.assert_array_equal(got["cost"], want["cost"], err_msg=what + ": cost")
    for f in ("parent", "link_cost", "children"):
        if f in got:
            np.testing.assert_array_equal(got[f], want[f], err_msg=what + ": " + f)
    if "rssi" in got:
        np.testing.assert_array_equal(N.bits(got["rssi"]), want["rssi"], err_msg=what + ": rssi bits")
    if totals is not None:
        assert totals == want["totals"], (what, totals, want["totals"])
