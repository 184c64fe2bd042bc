"""Reference of the neighbour query, on top of the untouched oracle: an O.tick over the non-SINR
log-distance parameters whose active records are nodes.packets(srcs) gives every potential link of those sources with its rssi; the
links are ranked in plain Python by the rule (rssi descending, ties by the far end's node index), for both directions.  No engine
code is involved and the library's exports are never the source of an expected value.  tests/test_neighbors_ref.py holds the
scenes' conditions for this reference alone, so that no GPU test passes vacuously."""
import types

import numpy as np

from oracle import oracle as O

HEARD_BY, HEARS = 0, 1
KS = (1, 2, 4, 8, 16)
NAN_BITS = 0x7FF8000000000000
# the oracle's log-distance defaults (pl0 40 dB, exponent 3, d0 1 m, sensitivity -95 dBm): txpower 0 reaches 68 m
PLAIN = {"ld_sigma_db": 0.0}
SHADOW = {"ld_sigma_db": 4.0, "ld_clip": 3.0, "ld_seed": 21}
SINR = {"ld_flags": 1, "ld_capture_db": 3.0, "ld_ifloor_dbm": -110.0}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(params):
    """the reference's medium: the scene's log-distance parameters WITHOUT the SINR flag (the rule says that it plays no part)"""
    kw = {k: v for k, v in params.items() if k not in ("ld_flags",)}
    return O.model(4, ld_flags=0, **kw)


def links(nd, params, direction, nodes=None):
    """all potential links of the listed nodes (None: of all) in one direction -> {node: [(rssi, far end)]}, unranked.
    HEARD_BY: a tick whose sources are the listed nodes.  HEARS: a tick whose sources are ALL nodes, over a copy of the table in
    which every receiver that is not listed is disabled (the oracle skips a disabled receiver before any arithmetic)."""
    mdl = _model(params)
    every = np.arange(nd.n, dtype=np.int32)
    asked = every if nodes is None else np.unique(np.asarray(nodes, dtype=np.int32))
    out = {int(j): [] for j in asked}
    if nd.n == 0 or len(asked) == 0:
        return out
    if direction == HEARD_BY:
        pk = nd.packets(asked)
        res = O.tick(mdl, nd, pk, cap=len(asked) * nd.n + 1)
        assert res.count == len(res.dst)
        for q, d, r in zip(res.pkt.tolist(), res.dst.tolist(), res.rssi.tolist()):
            out[int(asked[q])].append((r, d))
        return out
    tbl = nd
    if nodes is not None:
        tbl = O.NodeTable(nd.n)
        for name in ("x", "y", "z", "txpower", "channel", "rxprob", "txprob", "int_id"):
            setattr(tbl, name, np.array(getattr(nd, name)))
        keep = np.zeros(nd.n, dtype=np.uint8)
        keep[asked] = 1
        tbl.enabled = (np.asarray(nd.enabled, dtype=np.uint8) & keep).astype(np.uint8)
    pk = nd.packets(every)
    res = O.tick(mdl, tbl, pk, cap=len(asked) * nd.n + 1)
    assert res.count == len(res.dst)
    for q, d, r in zip(res.pkt.tolist(), res.dst.tolist(), res.rssi.tolist()):
        out[d].append((r, q))
    return out


def _copy(nd):
    tbl = O.NodeTable(nd.n)
    for name in ("x", "y", "z", "txpower", "channel", "enabled", "rxprob", "txprob", "int_id"):
        setattr(tbl, name, np.array(getattr(nd, name)))
    return tbl


def links_hears_large(nd, params, nodes):
    """HEARS links of a few nodes of a LARGE table, still from the oracle alone, in two ticks instead of one over all n sources.
    First the listed nodes transmit at the table's largest txpower to a table in which every radio is on and rxprob is 1: the
    receivers of node j are a superset of the transmitters j can hear (distance and shadowing deviate are symmetric in the pair, the
    rssi grows with txpower, channels are as they are).  Then those nodes transmit, as they are, to the listed receivers alone.
    tests/test_neighbors_ref.py holds this to links() on a small scene."""
    asked = np.unique(np.asarray(nodes, dtype=np.int32))
    out = {int(j): [] for j in asked}
    wide = _copy(nd)
    wide.enabled[:] = 1
    wide.rxprob[:] = 1.0
    wide.txpower[asked] = np.max(nd.txpower)
    res = O.tick(_model(params), wide, wide.packets(asked), cap=len(asked) * nd.n + 1)
    cand = np.unique(res.dst)
    if len(cand) == 0:
        return out
    tbl = _copy(nd)
    keep = np.zeros(nd.n, dtype=np.uint8)
    keep[asked] = 1
    tbl.enabled = (np.asarray(nd.enabled, dtype=np.uint8) & keep).astype(np.uint8)
    res = O.tick(_model(params), tbl, nd.packets(cand), cap=len(asked) * len(cand) + 1)
    for q, d, r in zip(res.pkt.tolist(), res.dst.tolist(), res.rssi.tolist()):
        out[d].append((r, int(cand[q])))
    return out


def rank(found, K):
    """the rule over one node's links [(rssi, far end)] -> (peers [K], rssi bits [K], degree)"""
    found = [f for f in found if f[0] == f[0]]  # (a NaN rssi is no link)
    order = sorted(found, key=lambda f: (-f[0], f[1]))
    peer = [f[1] for f in order[:K]] + [-1] * max(0, K - len(order))
    rb = [int(bits([f[0]])[0]) for f in order[:K]] + [NAN_BITS] * max(0, K - len(order))
    return peer, rb, len(found)


def rows(nd, params, direction, K, nodes=None, found=None):
    """the expected outputs for the listed nodes in list order (None: all, node order): peer int32[n][K], rssi bits uint64[n][K],
    degree int32[n]; an entry outside the table is an empty row.  found: links() of at least these nodes, computed before"""
    if found is None:
        ok = None if nodes is None else [j for j in np.asarray(nodes).tolist() if 0 <= j < nd.n]
        found = links(nd, params, direction, ok)
    asked = list(range(nd.n)) if nodes is None else [int(j) for j in np.asarray(nodes).tolist()]
    peer = np.full((len(asked), K), -1, dtype=np.int32)
    rb = np.full((len(asked), K), NAN_BITS, dtype=np.uint64)
    deg = np.zeros(len(asked), dtype=np.int32)
    for e, j in enumerate(asked):
        if 0 <= j < nd.n:
            peer[e], rb[e], deg[e] = rank(found[j], K)
    return peer, rb, deg


def same(got, want, what, K=None):
    """exact equality of a query's outputs {"peer", "rssi", "degree"} (rssi / degree may be missing) with rows()"""
    np.testing.assert_array_equal(got["peer"], want[0], err_msg=what + ": peer")
    if "rssi" in got:
        np.testing.assert_array_equal(bits(got["rssi"]).reshape(want[1].shape), want[1], err_msg=what + ": rssi bits")
    if "degree" in got:
        np.testing.assert_array_equal(got["degree"], want[2], err_msg=what + ": degree")


def host_result(nd, params, srcs):
    """one tick's host result as the engine lays it out (packet-major, dst ascending per packet), from the oracle: an object with
    count, pkt_offset, dst, rssi -- what Engine.neighbors_from_result takes"""
    srcs = np.asarray(srcs, dtype=np.int32)
    res = O.tick(_model(params), nd, nd.packets(srcs), cap=max(1, len(srcs)) * max(1, nd.n) + 1)
    assert (np.diff(res.pkt) >= 0).all()
    off = np.zeros(len(srcs) + 1, dtype=np.uint32)
    np.add.at(off, res.pkt.astype(np.int64) + 1, 1)
    return types.SimpleNamespace(count=int(res.count), pkt_offset=np.cumsum(off).astype(np.uint32), dst=res.dst.astype(np.int32),
                                 rssi=res.rssi.astype(np.float64), verdict=res.verdict, sinr=None, pkt_rssi=None)


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def _field(n, seed, side):
    """n nodes: three quarters uniform over side x side, a quarter in a dense patch (degrees from 0 to far above 16), three transmit
    powers"""
    rng = np.random.default_rng(seed)
    nd = O.NodeTable(n)
    dense = np.arange(n) % 4 == 0
    nd.x = np.where(dense, rng.uniform(0.30, 0.45, n), rng.uniform(0, 1, n)) * side
    nd.y = np.where(dense, rng.uniform(0.30, 0.45, n), rng.uniform(0, 1, n)) * side
    nd.z = np.zeros(n)
    nd.txpower = rng.choice([0.0, -6.0, 3.0], n)
    return nd


SPECIAL = 8  # the crafted nodes at the end of a rich table


def rich(n, seed, side=None):
    """a field of n - SPECIAL random nodes and, far to its right, the crafted ones: a source S with two receivers mirrored about it
    (an exact rssi tie without shadowing), a disabled receiver, an rxprob = 0 receiver and an other-channel receiver inside its
    reach, a louder neighbour (S's HEARS row differs from its HEARD_BY row), and a node out of everybody's reach"""
    assert n > SPECIAL + 8
    side = side if side is not None else float(np.sqrt((n - SPECIAL) * 2400.0))   # (some six links a node in the sparse part)
    base = _field(n - SPECIAL, seed, side)
    nd = O.NodeTable(n)
    k = n - SPECIAL
    for name in ("x", "y", "z", "txpower"):
        getattr(nd, name)[:k] = getattr(base, name)
    cx, cy = float(np.ceil(side)) + 400.0, 100.0
    S, A, B, OFF, DEAF, OTHER, LOUD, LONE = range(k, n)
    nd.x[S], nd.y[S] = cx, cy
    nd.x[A], nd.y[A] = cx - 8.0, cy
    nd.x[B], nd.y[B] = cx + 8.0, cy
    nd.x[OFF], nd.y[OFF] = cx, cy + 5.0
    nd.enabled[OFF] = 0
    nd.x[DEAF], nd.y[DEAF] = cx, cy - 5.0
    nd.rxprob[DEAF] = 0.0
    nd.x[OTHER], nd.y[OTHER] = cx + 3.0, cy + 3.0
    nd.channel[OTHER] = 11
    nd.x[LOUD], nd.y[LOUD] = cx, cy + 90.0   # out of S's reach (68 m at txpower 0), S inside its own (20 dB more: 316 m)
    nd.txpower[LOUD] = 20.0
    nd.x[LONE], nd.y[LONE] = cx + 5000.0, cy + 5000.0
    nd.txpower[k:LOUD] = 0.0
    nd.txpower[LONE] = 0.0
    return nd


def special(nd):
    k = nd.n - SPECIAL
    return dict(zip(("S", "A", "B", "OFF", "DEAF", "OTHER", "LOUD", "LONE"), range(k, nd.n)))


def tiny(n):
    """1, 2 or 3 nodes in a row, 10 m apart"""
    nd = O.NodeTable(n)
    nd.x = 10.0 * np.arange(n)
    nd.txpower = np.array([0.0, 3.0, -3.0])[:n]
    return nd


SCENES = {
    "one": (lambda: tiny(1), PLAIN), "two": (lambda: tiny(2), PLAIN), "three": (lambda: tiny(3), SHADOW),
    "n65": (lambda: rich(65, 4), PLAIN), "n65_shadow": (lambda: rich(65, 4), SHADOW),
    "n300": (lambda: rich(300, 13), PLAIN), "n300_shadow": (lambda: rich(300, 13), SHADOW),
    "n300_sinr": (lambda: rich(300, 13), dict(PLAIN, **SINR)), "n300_shadow_sinr": (lambda: rich(300, 14), dict(SHADOW, **SINR)),
}
RICH = ("n65", "n65_shadow", "n300", "n300_shadow", "n300_sinr", "n300_shadow_sinr")
_CACHE = {}


def scene(name):
    """-> (nd, params, {direction: links of all nodes}); computed once, shared and left unchanged"""
    if name not in _CACHE:
        make, params = SCENES[name]
        nd = make()
        _CACHE[name] = (nd, params, {d: links(nd, params, d) for d in (HEARD_BY, HEARS)})
    return _CACHE[name]


def large(n, seed=9, n_off=70):
    """a rich table of n nodes for list queries: n_off radios off (more than one wave's round of the list the HEARS walk keeps of
    them) -> (nd, the query list: the nodes nearest the field's corners and centre, the crafted source, a radio that is off, the
    loud node, the lone node)"""
    nd = rich(n, seed)
    rng = np.random.default_rng(seed + 1)
    k = n - SPECIAL
    nd.enabled[rng.choice(k, n_off, replace=False)] = 0
    side = float(np.sqrt(k * 2400.0))
    spots = [(0, 0), (side, 0), (0, side), (side, side), (side / 2, side / 2), (0.375 * side, 0.375 * side)]
    near = [int(np.argmin((nd.x[:k] - px) ** 2 + (nd.y[:k] - py) ** 2)) for px, py in spots]
    sp = special(nd)
    off = int(np.flatnonzero(nd.enabled[:k] == 0)[0])
    ask = np.array(sorted(set(near + [sp["S"], sp["OFF"], sp["LOUD"], sp["LONE"], off])), dtype=np.int32)
    return nd, ask
