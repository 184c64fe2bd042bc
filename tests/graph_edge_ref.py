"""Scenes for the parts of the three graph queries (rm_neighbors.hip, rm_hops.hip, rm_routes.hip)
that random flat fields never reach: a three-dimensional lattice whose links tie in whole shells and end exactly on the level, a
frame whose fp32 slack lies just under the limit of the boxes path (and just over it), a table of channels that alias in the masks,
radios that are off, non-finite powers and odd receive probabilities, table sizes around the group of 64 and the box of 1024, root
lists longer than one stride of the seeding kernels, a hub whose degree is K - 1, K and K + 1, and a route whose first label is
exactly 129 above the cost a later round offers, with links that cost exactly 431 and 1787 behind it.  Expected values come only from neighbors_ref.links / rows, hops_ref.tree and
routes_ref.tree (the oracle's potential links); no engine code is involved and the library's exports are never called.
tests/test_graph_edge_ref.py holds every scene to its conditions, tests/test_gpu_graph_edges.py runs them."""
import numpy as np

from oracle import oracle as O

import hops_ref as H
import neighbors_ref as N
import routes_ref as R

HEARD_BY, HEARS, DIRS = H.HEARD_BY, H.HEARS, H.DIRS
INF = float("inf")
STEP = 30.0                                    # the lattices' spacing in metres
MARGINAL = dict(N.PLAIN, ld_sensitivity_dbm=-103.0)
Q = {"NONE": dict(R.SETS["NONE"][0]), "OQPSK": dict(R.SETS["OQPSK"][0])}      # us_per_bit 4, air_us 4064, cap 1024
CAPS = (128, 129, 430, 431, 1786, 1787, 65535)
ROUTE_SHELLS = (6, 7, 10)                      # the shells of the lattice whose own rssi the route tests take as min_rssi_dbm
_CACHE = {}


def memo(key, make):
    """computed once, shared and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def pair_rssi(d):
    """the oracle's own rssi, bit for bit, of two txpower-0 nodes d metres apart"""
    def make():
        nd = O.NodeTable(2)
        nd.x[:] = (0.0, d)
        nd.txpower[:] = 0.0
        (r, far), = N.links(nd, dict(N.PLAIN, ld_sensitivity_dbm=-1000.0), HEARD_BY, [0])[0]
        assert far == 1
        return float(r)
    return memo(("pair", float(d)), make)


def level(d):
    """the unshadowed medium whose sensitivity is exactly the rssi of a pair d metres apart: such a pair is a link, at the level"""
    return dict(N.PLAIN, ld_sensitivity_dbm=pair_rssi(d))


MEDIA = {"LEVEL": lambda: level(3 * STEP), "MARGINAL": lambda: MARGINAL, "LEVEL30": lambda: level(STEP), "PLAIN": lambda: N.PLAIN}


def table(pos, seed=None):
    """the points as a node table, txpower 0; seed: the points are dealt to the node indices by a seeded permutation, so that the
    rule's tie-break by node index disagrees with every spatial order -> (table, at: the node at point k)"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    at = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    nd = O.NodeTable(n)
    nd.x[at], nd.y[at], nd.z[at] = pos[:, 0], pos[:, 1], pos[:, 2]
    nd.txpower[:] = 0.0
    return nd, at


def sites(nx, ny, nz):
    """the points of an nx x ny x nz lattice, x fastest"""
    i = np.arange(nx * ny * nz)
    return STEP * np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], axis=1).astype(np.float64)


def both(nd, params):
    return {d: N.links(nd, params, d) for d in DIRS}


def shells(found, node):
    """the distinct rssi values of a node's links, strongest first, with the number of links at each"""
    vals = sorted({r for r, _ in found[node]}, reverse=True)
    return [(v, sum(1 for r, _ in found[node] if r == v)) for v in vals]


def up(r):
    return float(np.nextafter(r, INF))


# ---- 1. lattice3d ------------------------------------------------------------------------------------------------------------------
SIDE = 9


def lattice3d_table():
    """9 x 9 x 9 points, 30 m apart, dealt to the node indices by a seeded permutation -> (table, at)"""
    return memo("lattice3d", lambda: table(sites(SIDE, SIDE, SIDE), seed=0x3D))


def site(ix, iy, iz, side=SIDE):
    return ix + side * (iy + side * iz)


def lattice3d(medium):
    """-> (table, the medium's parameters, {direction: links of all nodes})"""
    def make():
        nd, _ = lattice3d_table()
        params = MEDIA[medium]()
        return nd, params, both(nd, params)
    return memo(("lattice3d", medium), make)


def lattice3d_roots():
    """the root sets of the lattice: a corner, the centre, every node, two opposite corners"""
    nd, at = lattice3d_table()
    m = SIDE // 2
    return {"corner": [int(at[0])], "centre": [int(at[site(m, m, m)])], "all": list(range(nd.n)), "corners": [int(at[0]), int(at[nd.n - 1])]}


def interior():
    """the nodes at least three steps from every face: their links reach every shell of both media whole up to 90 m"""
    _, at = lattice3d_table()
    return [int(at[site(x, y, z)]) for x in range(3, SIDE - 3) for y in range(3, SIDE - 3) for z in range(3, SIDE - 3)]


def hop_tree(medium, d, label, min_rssi=-INF):
    nd, _, found = lattice3d(medium)
    return memo(("hop", medium, d, label, min_rssi), lambda: H.tree(nd.n, found[d], lattice3d_roots()[label], min_rssi))


def route_tree(medium, d, label, kind, **kw):
    nd, _, found = lattice3d(medium)
    q = dict(Q[kind], **kw)
    return memo(("route", medium, d, label, kind, tuple(sorted(kw.items()))), lambda: R.tree(nd.n, found[d], lattice3d_roots()[label], q))


# ---- 2. wide -----------------------------------------------------------------------------------------------------------------------
WIDE_L = {"boxes": 2.3e5, "scan": 2.6e5}       # the cluster's corner: an fp32 slack of about 0.0475 m, and of about 0.054 m
N_PROBES = 64


def probes(L):
    """For each of 64 seeded directions u the scalar t of src + t * u is bisected over [29, 31] with the oracle (one tick of the
    source over all 64 candidates a step) down to two adjacent doubles: the last t that is a link and the next one, which is none.
    -> (the source's position, in-probes [64][3], out-probes [64][3])"""
    def make():
        rng = np.random.default_rng(0x71DE)
        u = rng.normal(size=(N_PROBES, 3))
        u /= np.sqrt((u * u).sum(axis=1))[:, None]
        src = np.array([L, L, L])
        params = level(STEP)

        def heard(t):
            nd, _ = table(np.concatenate([src[None, :], src[None, :] + t[:, None] * u]))
            got = np.zeros(N_PROBES, dtype=bool)
            got[[far - 1 for _, far in N.links(nd, params, HEARD_BY, [0])[0]]] = True
            return got

        lo, hi = np.full(N_PROBES, 29.0), np.full(N_PROBES, 31.0)
        assert heard(lo).all() and not heard(hi).any()
        while True:
            mid = lo + (hi - lo) / 2
            live = (mid > lo) & (mid < hi)
            if not live.any():
                break
            h = heard(np.where(live, mid, lo))
            lo, hi = np.where(live & h, mid, lo), np.where(live & ~h, mid, hi)
        assert (np.nextafter(lo, INF) == hi).all()
        return src, src[None, :] + lo[:, None] * u, src[None, :] + hi[:, None] * u
    return memo(("probes", L), make)


def wide(path):
    """the lattice's nodes, then the source, the in-probes and the out-probes -> (table, parameters, {direction: links of all nodes},
    {"src", "in", "out"}: node indices)"""
    def make():
        nd0, _ = lattice3d_table()
        src, pin, pout = probes(WIDE_L[path])
        pos = np.concatenate([np.stack([nd0.x, nd0.y, nd0.z], axis=1), src[None, :], pin, pout])
        nd, _ = table(pos)
        k = nd0.n
        who = {"src": k, "in": list(range(k + 1, k + 1 + N_PROBES)), "out": list(range(k + 1 + N_PROBES, k + 1 + 2 * N_PROBES))}
        params = level(STEP)
        return nd, params, both(nd, params), who
    return memo(("wide", path), make)


def frame(nd):
    """the bound of the fp32 frame as DESIGN.md's "Pre-filter" gives it (half the table's largest extent) and the slack that follows
    from it: 4 * sqrt(3) * 2^-24 * bound"""
    bound = max(float(np.max(c) - np.min(c)) / 2.0 for c in (nd.x, nd.y, nd.z))
    return bound, 4.0 * np.sqrt(3.0) * 2.0 ** -24 * bound


# ---- 3. specials -------------------------------------------------------------------------------------------------------------------
N_OFF = 70
ODD_POWER = (float("nan"), INF, -INF, 1e300)
ODD_RXPROB = (float("nan"), -0.0, -1.0, 5e-324)


def specials():
    """the lattice under MARGINAL with four channels that share one bit of a 32-bit mask (one of them negative), 70 radios off
    over all four, and eight nodes with a non-finite power or an odd receive probability
    -> (table, parameters, {"power": nodes, "rxprob": nodes, "off": nodes})"""
    def make():
        nd = N._copy(lattice3d_table()[0])
        rng = np.random.default_rng(0x5BEC)
        c = int(nd.channel[0])
        nd.channel[:] = c + np.array([0, 32, -32, 64])[np.arange(nd.n) % 4]
        off = np.sort(rng.choice(nd.n, N_OFF, replace=False))
        nd.enabled[off] = 0
        inner = [j for j in interior() if nd.enabled[j]]
        odd = rng.choice(inner, 8, replace=False)
        nd.txpower[odd[:4]] = ODD_POWER
        nd.rxprob[odd[4:]] = ODD_RXPROB
        return nd, MARGINAL, {"power": [int(j) for j in odd[:4]], "rxprob": [int(j) for j in odd[4:]], "off": [int(j) for j in off]}
    return memo("specials", make)


def specials_links():
    nd, params, _ = specials()
    return memo("specials links", lambda: both(nd, params))


# ---- 4. sizes ----------------------------------------------------------------------------------------------------------------------
SIZES = (65, 1023, 1024, 1025)


def sizes(n):
    """the first n - 1 points of a 16 x 8 x 8 lattice and one more point a diagonal step outside its first corner, dealt to the node
    indices by a seeded permutation, under MARGINAL -> (table, parameters, {direction: links of all nodes}, at)"""
    def make():
        pos = np.concatenate([sites(16, 8, 8)[:n - 1], [[-STEP, -STEP, -STEP]]])
        nd, at = table(pos, seed=n)
        return nd, MARGINAL, both(nd, MARGINAL), at
    return memo(("sizes", n), make)


# ---- 5. many_roots -----------------------------------------------------------------------------------------------------------------
STRIDE = 64 * 256                                # the entries one round of k_hop_seed / k_route_seed takes


def root_lists():
    """root lists over the lattice's nodes, drawn with repetition from 100 nodes of which three ("late") are kept out of the first
    stride: "16384" fills one stride, "16385" holds late[0] alone in the second, "40000" holds late[1] in the second and late[2] in
    the third, "every" is every node 23 times over, node by node (the nodes from 713 on lie behind the first stride); "outside" is
    the device form's list: "16384" and behind it entries outside the table around late[0] -> ({label: list}, late)"""
    def make():
        n = lattice3d_table()[0].n
        rng = np.random.default_rng(0x4007)
        pool = rng.choice(n, 100, replace=False).astype(np.int32)
        early, late = pool[:97], pool[97:]
        a = rng.choice(early, STRIDE).astype(np.int32)
        c = rng.choice(early, 40000).astype(np.int32)
        c[STRIDE + 5], c[39999] = late[1], late[2]
        lists = {"16384": a, "16385": np.concatenate([a, late[:1]]), "40000": c, "every": np.repeat(np.arange(n, dtype=np.int32), 23),
                 "outside": np.concatenate([a, np.array([-1, n, late[0], 2 ** 31 - 1, -1], dtype=np.int32)])}
        return lists, [int(j) for j in late]
    return memo("root lists", make)


# ---- 6. hub ------------------------------------------------------------------------------------------------------------------------
HUB_M = (15, 16, 17)
N_FILL = 70


def _fillers(k):
    """k points 500 m apart on a line far from everything: out of everybody's reach under every medium here"""
    return np.stack([5000.0 + 500.0 * np.arange(k), np.full(k, -5000.0), np.full(k, 700.0)], axis=1)


def hub(m):
    """a hub, m of the 6 + 12 lattice points 30 m and 30 * sqrt(2) m from it (all six of the first shell), and fillers out of reach
    that make the table larger than 64 nodes, under the oracle's default medium -> (table, parameters, the hub's node)"""
    def make():
        near = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if 1 <= x * x + y * y + z * z <= 2]
        near.sort(key=lambda p: p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        pos = np.concatenate([[[0.0, 0.0, 0.0]], STEP * np.array(near[:m], dtype=np.float64), _fillers(N_FILL)])
        nd, at = table(pos, seed=100 + m)
        return nd, N.PLAIN, int(at[0])
    return memo(("hub", m), make)


# ---- 7. bounds ---------------------------------------------------------------------------------------------------------------------
RELAX_DIRECT = 385                               # the root's own link to V: 129 above what the third round offers


def bounds():
    """root R, A, P and V under MARGINAL / OQPSK: R - A, A - P and P - V cost 128 each, R - V is a direct link of cost exactly 385 (V's
    distance is bisected with the oracle's rssi and the reference's cost), R - P costs more than 256 and A - V is no link.  V is
    labelled 385 in the first round and P 256 in the second; in the third P offers 384 to a node whose cost is cost[P] + 129.
    Behind V a chain whose links are the only way on: X, one step of the lattice's 431 shell from V, and Y, one step of its 1787
    shell from X -- a cap of 430 or 431 decides X, one of 1786 or 1787 decides Y.
    -> (table, parameters, {direction: links}, {"R", "A", "P", "V", "X", "Y"})"""
    def make():
        q = dict(Q["OQPSK"], max_link_cost=65535)
        cost = lambda x: R.link_cost(q, pair_rssi(x))
        lo, hi = 3.4 * STEP, 3.65 * STEP         # (between the shells that cost 204 and 431)
        assert cost(lo) < RELAX_DIRECT < cost(hi)
        while cost(lo + (hi - lo) / 2) != RELAX_DIRECT:
            mid = lo + (hi - lo) / 2
            assert lo < mid < hi
            lo, hi = (mid, hi) if cost(mid) < RELAX_DIRECT else (lo, mid)
        x = lo + (hi - lo) / 2
        vx = [x + 3 * STEP, -2 * STEP, 0.0]
        vy = [vx[0] + 3 * STEP, vx[1] - 2 * STEP, STEP]
        pos = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 80.0, 0.0], [78.0, 78.0, 0.0], [x, 0.0, 0.0], vx, vy], _fillers(N_FILL)])
        nd, at = table(pos, seed=0x129)
        return nd, MARGINAL, both(nd, MARGINAL), dict(zip("RAPVXY", (int(j) for j in at[:6])))
    return memo("bounds", make)
