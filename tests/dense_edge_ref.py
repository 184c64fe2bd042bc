"""Scenes and expected values for the parts of the dense tick (rm_dense.hip) that uniform flat scenes never
reach: receivers exactly on the range's edge and inside the relative band of 1e-9 around range^2 that dense_eval decides by the
reference's own steps, the same edge pairs in three dimensions, receiver and transmit probabilities outside (0, 1), node and frame
counts around the chunk of 1024 nodes, the wave of 64 and the group of eight frames, index partitions that begin or end inside a
wave, ticks of padding records, cell counts on both sides of 8192, and a 0/1 matrix.  Expected values come from the oracle alone
(O.tick_mt: no tick here needs a draw); no engine code is involved.  tests/test_dense_edge_ref.py holds every scene to its
conditions, tests/test_gpu_dense_edges.py runs them."""
import itertools

import numpy as np

_CACHE = {}
TICK = 1000
KINDS = {"null": 0, "udgm": 1, "udgm_const": 2, "n2n": 3, "logdist": 4}


class Tick:
    """A source list with one start and one air time; -1 in the list is a padding slot (a slot of the tick without a packet)."""

    def __init__(self, src, k=0, air=320):
        self.src = np.asarray(src, dtype=np.int32)
        self.t_begin, self.t_end, self.start, self.air = k * TICK, (k + 1) * TICK, k * TICK, air
        real = self.src[self.src >= 0]
        assert len(self.src) and len(np.unique(real)) == len(real), "a tick's nodes are distinct"

    def __len__(self):
        return len(self.src)

    def packets(self, nd):
        """one record per slot; a padding slot's record is node 0's with src = -1"""
        p = nd.packets(np.maximum(self.src, 0), self.start, self.air)
        p["src"] = self.src
        return p


class Scene:
    """A node table, a medium, ticks, an index partition of receivers (first, count) and whether only the knob (RM_DENSE_TICK=1)
    sends the ticks the dense way (`force`); `dense`: the tick is meant to take the dense form (None: the scene does not say)."""

    def __init__(self, name, nd, kind, params, ticks, force, part=None, matrix=None, dense=True):
        self.name, self.nd, self.kind, self.params, self.ticks, self.force = name, nd, kind, dict(params), ticks, force
        self.part, self.matrix, self.dense = part or (0, nd.n), matrix, dense
        assert nd.n <= 5000 and 0 <= self.part[0] and self.part[1] >= 1 and self.part[0] + self.part[1] <= nd.n

    def model(self, O):
        kw = dict(self.params)
        if self.matrix is not None:
            kw["n2n_matrix"] = self.matrix
        return O.model(KINDS[self.kind], **kw)


class Expected:
    """The oracle's result of one tick in the engine's terms: packets numbered by slot (padding slots are packets without links),
    receivers of the scene's partition only, pkt_offset per slot, and `real`: the slots that hold a packet (a padding slot's
    Tx-failure flag is given as 0: the oracle knows no such packet, and the engine's flag of it is not compared)."""

    def __init__(self, O, sc, tk):
        recs = tk.packets(sc.nd)
        self.real = recs["src"] >= 0
        slot = np.flatnonzero(self.real)
        n_real = len(slot)
        pint = np.zeros(len(recs), dtype=np.uint8)
        if n_real:
            cap = min(n_real * sc.nd.n, 1 << 22)
            res = O.tick_mt(sc.model(O), sc.nd, recs[self.real], cap=cap)       # (raises if the tick needs a draw)
            assert res.count <= cap
            pkt, dst, verdict, rssi, sinr = slot[res.pkt].astype(np.int32), res.dst, res.verdict, res.rssi, res.sinr
            pint[slot] = res.pkt_interference
        else:
            pkt = dst = np.zeros(0, dtype=np.int32)
            verdict, rssi, sinr = np.zeros(0, dtype=np.uint8), np.zeros(0), np.zeros(0)
        first, count = sc.part
        keep = (dst >= first) & (dst < first + count)
        self.pkt, self.dst, self.verdict, self.rssi, self.sinr = pkt[keep], dst[keep], verdict[keep], rssi[keep], sinr[keep]
        self.count = int(keep.sum())
        self.pkt_interference = pint
        self.pkt_offset = np.searchsorted(self.pkt, np.arange(len(recs) + 1)).astype(np.uint32)
        for a in (self.pkt, self.dst, self.verdict, self.rssi, self.sinr, self.pkt_interference, self.pkt_offset):
            a.setflags(write=False)

    def heard(self, n_slots, first, count):
        """bool [slot][node of the partition]: the oracle's heard sets as the lane masks hold them"""
        m = np.zeros((n_slots, count), dtype=bool)
        m[self.pkt, self.dst - first] = True
        return m


def distance(O, a, b):
    """the reference's distance (Position.getDistanceTo: three squares, one sum, one root), by the oracle"""
    return O.lib().orc_distance(float(a[0]), float(a[1]), float(a[2]), float(b[0]), float(b[1]), float(b[2]))


# ---- 1. lattice3d ----------------------------------------------------------------------------------------------------------------------
LATTICE = (16, 16, 8)
LATTICE_CHANNELS = (26, 58)          # the same bit of a 32-bit channel mask: only the exact compare separates them
LATTICE_MODELS = {"udgm7": ("udgm", {"udgm_transmission_range": 7.0}), "udgm9": ("udgm", {"udgm_transmission_range": 9.0}),
                  "const7": ("udgm_const", {"const_range": 7.0}), "const9": ("udgm_const", {"const_range": 9.0})}
PROB_RX = (1.0, 0.0, -0.0, -0.5, 2.0, 1e300)       # rm_nodes_upload takes every double as a probability: none is dropped
PROB_TX = (1.0, 0.0, -1.0, 1.5)
PROB_MODELS = {"udgm": ("udgm", {"udgm_transmission_range": 7.0, "udgm_success_ratio_rx": 1.0}),
               "const": ("udgm_const", {"const_range": 7.0}), "null": ("null", {})}


def lattice_table(O, probs=False):
    """16 x 16 x 8 integer lattice at 1 m pitch (x fastest): 2048 nodes, two chunks of the dense tick; 2 % of the radios off, two
    channels, about 150 sources.  Every squared distance is an integer: d == 7 and d == 9 are met exactly, most often with
    dz != 0 (7^2 = 2^2 + 3^2 + 6^2, 9^2 = 1^2 + 4^2 + 8^2 = 4^2 + 4^2 + 7^2 ...)."""
    key = ("lattice", probs)
    if key not in _CACHE:
        rng = np.random.default_rng(0x3D)
        nx, ny, nz = LATTICE
        n = nx * ny * nz
        nd = O.NodeTable(n)
        i = np.arange(n)
        nd.x[:], nd.y[:], nd.z[:] = i % nx, (i // nx) % ny, i // (nx * ny)
        nd.channel[:] = rng.choice(LATTICE_CHANNELS, n)
        nd.enabled[rng.choice(n, n // 50, replace=False)] = 0
        nd.txpower[:] = rng.uniform(-10.0, 0.0, n)
        src = np.sort(rng.choice(n, 150, replace=False)).astype(np.int32)
        if probs:
            nd.rxprob[:] = rng.choice(PROB_RX, n)
            nd.txprob[src] = np.resize(PROB_TX, len(src))[rng.permutation(len(src))]
        _CACHE[key] = (nd, src)
    return _CACHE[key]


def lattice3d(O, which):
    nd, src = lattice_table(O)
    kind, params = LATTICE_MODELS[which]
    return Scene("lattice3d/" + which, nd, kind, params, [Tick(src)], force=False)


def probs(O, which):
    nd, src = lattice_table(O, probs=True)
    kind, params = PROB_MODELS[which]
    return Scene("probs/" + which, nd, kind, params, [Tick(src)], force=False)


# ---- 2. band ---------------------------------------------------------------------------------------------------------------------------
BAND_RANGE = 50.0
BAND_ORIGINS = {"near": (0.0, 0.0, 0.0), "far": (1.0e6, -3.0e5, 40.0)}
ULP = float(np.spacing(BAND_RANGE)) / BAND_RANGE            # "one ulp" as a relative step of the range
BAND_E = (0.0, ULP, -ULP, 1e-12, -1e-12, 4e-10, -4e-10, 6e-10, -6e-10, 2e-9, -2e-9)
BAND_DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2 / 7, 3 / 7, 6 / 7), (-2 / 7, -3 / 7, -6 / 7))
BAND_MODELS = {"udgm50": ("udgm", {"udgm_transmission_range": 50.0}), "udgm-50": ("udgm", {"udgm_transmission_range": -50.0}),
               "udgm0": ("udgm", {"udgm_transmission_range": 0.0}), "const50": ("udgm_const", {"const_range": 50.0}),
               "const0": ("udgm_const", {"const_range": 0.0})}
BAND_N, BAND_FIRST_PROBE = 1100, 980       # the probes lie across the chunk boundary at node 1024


def _place(O, origin, direction, e):
    """A point whose distance from `origin` BY THE REFERENCE'S ARITHMETIC is on the side of the range that `e` names (equal to the
    range for e == 0) and as near to range * (1 + e) as the coordinates allow: around a far origin a coordinate moves in steps of
    1e-10, so the nearest candidates are searched -- a few ulps of every coordinate that is not the origin's."""
    o, u = np.array(origin), np.array(direction, dtype=np.float64)
    want = BAND_RANGE * (1.0 + e) if abs(e) != ULP else float(np.nextafter(BAND_RANGE, np.inf if e > 0 else -np.inf))
    base = o + u * want
    free = [a for a in range(3) if u[a] != 0.0]
    last = free[-1]                                # (z on the diagonal: the coordinate with the finest steps around the far origin)

    def moved(v, k):
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        return v

    best = None
    for ks in itertools.product(range(-3, 4), repeat=len(free) - 1):
        p = base.copy()
        for a, k in zip(free, ks):
            p[a] = moved(p[a], k)
        # the last coordinate makes up for what the others' steps changed, then moves by a few ulps itself
        rest = want * want - sum((p[a] - o[a]) ** 2 for a in free[:-1])
        p[last] = o[last] + np.sign(u[last]) * np.sqrt(rest)
        for k in range(-24, 25):
            q = p.copy()
            q[last] = moved(p[last], k)
            d = distance(O, o, q)
            if np.sign(d - BAND_RANGE) != np.sign(e):
                continue
            err = abs(d - want)
            if best is None or err < best[0]:
                best = (err, q, d)
    assert best is not None, (origin, direction, e)
    return best[1], best[2]


def band_table(O, origin):
    """node 0: the source, at the origin; two receivers at its very place; the probes (every direction, every e) from node 980 on;
    the rest far away (1 to 3 km), where nobody hears anybody.  -> (table, probes: node, direction, e, the oracle's distance)"""
    key = ("band", origin)
    if key not in _CACHE:
        rng = np.random.default_rng(0xBA)
        o = np.array(BAND_ORIGINS[origin])
        nd = O.NodeTable(BAND_N)
        far = rng.uniform(1000.0, 3000.0, (BAND_N, 3)) * rng.choice([-1.0, 1.0], (BAND_N, 3))
        nd.x[:], nd.y[:], nd.z[:] = o[0] + far[:, 0], o[1] + far[:, 1], o[2] + far[:, 2]
        nd.txpower[:] = rng.uniform(-10.0, 0.0, BAND_N)
        for j in (0, 1, 1030):                        # the source and its two co-located receivers (one in each chunk)
            nd.x[j], nd.y[j], nd.z[j] = o
        probes, j = [], BAND_FIRST_PROBE
        for u in BAND_DIRS:
            for e in BAND_E:
                if j == 1030:
                    j += 1
                p, d = _place(O, o, u, e)
                nd.x[j], nd.y[j], nd.z[j] = p
                probes.append((j, u, e, d))
                j += 1
        assert j <= BAND_N
        _CACHE[key] = (nd, probes)
    return _CACHE[key]


BAND_SOURCES = (0, 500, 1099)        # the source at the origin and two far nodes (more than one frame in the tick)


def band(O, origin, which):
    nd, _ = band_table(O, origin)
    kind, params = BAND_MODELS[which]
    return Scene("band/%s/%s" % (origin, which), nd, kind, params, [Tick(BAND_SOURCES)], force=True)


# The sum of squares and the distance do not cross the range together: around range 9 the root of 81 +- 1 ulp rounds to 9 itself
# (half an ulp of 9 is more than the root moves), so a receiver with s > range^2 is still at d == range: in for UDGM, out for
# constant loss -- and one with s < range^2 is NOT inside the constant-loss range.  Only the reference's steps decide these.
SUM9_BASES = ((1.0, 4.0, 8.0), (4.0, 4.0, 7.0), (3.0, 6.0, 6.0))
SUM9_MODELS = {"udgm9": ("udgm", {"udgm_transmission_range": 9.0}), "const9": ("udgm_const", {"const_range": 9.0})}


def sum_of_squares(a, b):
    """the sum the reference takes the root of (Position.getDistanceTo), one rounding at a time"""
    dx, dy, dz = float(a[0]) - float(b[0]), float(a[1]) - float(b[1]), float(a[2]) - float(b[2])
    return (dx * dx + dy * dy) + dz * dz


def sum9_table(O):
    """-> (table, probes: node, side of 81 the sum lies on (+1, 0, -1)); every probe is at d == 9 by the reference's arithmetic"""
    key = ("sum9",)
    if key not in _CACHE:
        rng = np.random.default_rng(0x99)
        nd = O.NodeTable(BAND_N)
        far = rng.uniform(1000.0, 3000.0, (BAND_N, 3)) * rng.choice([-1.0, 1.0], (BAND_N, 3))
        nd.x[:], nd.y[:], nd.z[:] = far[:, 0], far[:, 1], far[:, 2]
        nd.x[0] = nd.y[0] = nd.z[0] = 0.0
        probes, j = [], 1018
        for base in SUM9_BASES:
            for side in (0, 1, -1):
                x, want = base[0], float(np.nextafter(81.0, np.inf * side)) if side else 81.0
                for _ in range(400):
                    p = (x, base[1], base[2])
                    if sum_of_squares(p, (0, 0, 0)) == want and distance(O, (0, 0, 0), p) == 9.0:
                        break
                    x = float(np.nextafter(x, np.inf * side))
                else:
                    raise AssertionError((base, side))
                nd.x[j], nd.y[j], nd.z[j] = p
                probes.append((j, side))
                j += 1
        _CACHE[key] = (nd, probes)
    return _CACHE[key]


def sum9(O, which):
    nd, _ = sum9_table(O)
    kind, params = SUM9_MODELS[which]
    return Scene("sum9/" + which, nd, kind, params, [Tick(BAND_SOURCES)], force=True)


# ---- 3. shapes -------------------------------------------------------------------------------------------------------------------------
# every n with two frame counts, every frame count with (at least) two n; a frame count is capped at n
SHAPES = ((1, 1), (2, 1), (2, 7), (63, 7), (63, 8), (64, 8), (64, 9), (65, 9), (65, 17), (1023, 1), (1023, 17), (1024, 7), (1024, 8),
          (1025, 8), (1025, 9), (2049, 1), (2049, 17))
SHAPE_MODELS = {"null": ("null", {}), "udgm": ("udgm", {"udgm_transmission_range": 400.0})}
PARTS = ((0, 1), (1, 1), (63, 2), (1000, 48), (1023, 1026), (5, 2049 - 5))
PART_OFF = (300, 70)                 # every radio of these nodes is off in the table of 2049


def shape_table(O, n):
    key = ("shape", n)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + n)
        nd = O.NodeTable(n)
        nd.x[:], nd.y[:], nd.z[:] = rng.uniform(0, 100.0, n), rng.uniform(0, 100.0, n), rng.uniform(0, 20.0, n)
        nd.channel[:] = rng.choice((26, 11), n)
        nd.enabled[:] = rng.uniform(size=n) >= 0.1
        nd.txpower[:] = rng.uniform(-10.0, 0.0, n)
        if n == 2049:
            nd.enabled[PART_OFF[0]:PART_OFF[0] + PART_OFF[1]] = 0
        _CACHE[key] = nd
    return _CACHE[key]


def _sources(n, t, seed):
    return np.sort(np.random.default_rng(seed).choice(n, min(t, n), replace=False)).astype(np.int32)


def shapes(O, model, n, t):
    kind, params = SHAPE_MODELS[model]
    return Scene("shapes/%s/%d/%d" % (model, n, t), shape_table(O, n), kind, params, [Tick(_sources(n, t, 7 * n + t))], force=True)


def parts(O, model, what):
    """the table of 2049 nodes with an index partition of receivers, or with padding slots in the tick"""
    kind, params = SHAPE_MODELS[model]
    nd = shape_table(O, 2049)
    src, part = _sources(2049, 17, 7 * 2049 + 17), None          # (the sources of shapes/*/2049/17)
    if what == "off":
        part = PART_OFF
    elif what == "outside":                     # no source is a receiver of the partition
        part = (1000, 48)
        src = np.concatenate([_sources(1000, 5, 5), 1048 + _sources(1001, 4, 6)]).astype(np.int32)
    elif what == "padding-only":
        src = np.full(9, -1, dtype=np.int32)
    elif what == "padding":
        src = src.copy()
        src[[0, 5, 8, 16]] = -1
    elif what == "padding-part":
        part = (1023, 1026)
        src = src.copy()
        src[2::3] = -1
    else:
        part = tuple(int(v) for v in what.split("-"))
        assert part in PARTS
    return Scene("parts/%s/%s" % (model, what), nd, kind, params, [Tick(src)], force=True, part=part)


PART_NAMES = ["%d-%d" % p for p in PARTS] + ["off", "outside", "padding-only", "padding", "padding-part"]


# ---- 4. cells --------------------------------------------------------------------------------------------------------------------------
CELLS = {"8190": (5000, 1638), "8192": (4096, 2048), "8195": (5000, 1639)}       # (nodes, frames): frames * chunks cells
CELLS_PARAMS = {"udgm_transmission_range": 30.0}


def cells_table(O, n):
    key = ("cells", n)
    if key not in _CACHE:
        rng = np.random.default_rng(n)
        nd = O.NodeTable(n)
        nd.x[:], nd.y[:], nd.z[:] = rng.uniform(0, 300.0, n), rng.uniform(0, 300.0, n), rng.uniform(0, 10.0, n)
        nd.channel[:] = rng.choice((26, 11), n)
        nd.enabled[rng.choice(n, n // 40, replace=False)] = 0
        nd.txpower[:] = rng.uniform(-10.0, 0.0, n)
        _CACHE[key] = nd
    return _CACHE[key]


def cells(O, which):
    n, t = CELLS[which]
    return Scene("cells/" + which, cells_table(O, n), "udgm", CELLS_PARAMS, [Tick(_sources(n, t, t))], force=True)


def cells_small(O, k):
    """a few frames on the table of 5000 nodes (the ticks between the large ones of a sequence)"""
    return Scene("cells/small/%d" % k, cells_table(O, 5000), "udgm", CELLS_PARAMS, [Tick(_sources(5000, (40, 9, 33, 64)[k], 77 + k))], force=True)


CULLED = {"logdist": ("logdist", {"ld_sensitivity_dbm": -82.0}), "udgm": ("udgm", CELLS_PARAMS)}


def culled(O, model, k):
    """a tick of the same table that takes a culled form: the log-distance medium (never dense), or the unit disc with the knob off"""
    kind, params = CULLED[model]
    return Scene("culled/%s/%d" % (model, k), cells_table(O, 5000), kind, params, [Tick(_sources(5000, 50 + 7 * k, 500 + k))], force=False, dense=False)


# ---- 5. n2n01 --------------------------------------------------------------------------------------------------------------------------
def n2n01(O):
    """300 nodes, a matrix of zeros and ones over the ids 1 .. 298, receiver and transmit probabilities of 0 or 1: no link of this
    medium can draw.  Two nodes carry ids outside the matrix (0 and 1000): they hear nobody and nobody hears them."""
    rng = np.random.default_rng(0x22)
    n, m = 300, 298
    nd = O.NodeTable(n)
    nd.x[:], nd.y[:] = rng.uniform(0, 100.0, n), rng.uniform(0, 100.0, n)
    nd.rxprob[:] = rng.choice((0.0, 1.0, 1.0, 1.0), n)
    nd.txprob[:] = rng.choice((0.0, 1.0, 1.0), n)
    nd.enabled[rng.choice(n, 6, replace=False)] = 0
    nd.txpower[:] = rng.uniform(-10.0, 0.0, n)
    ids = rng.permutation(np.arange(1, n + 1)).astype(np.int32)
    outside = np.flatnonzero(ids > m)
    ids[outside[0]], ids[outside[1]] = 0, 1000
    nd.int_id[:] = ids
    matrix = (rng.uniform(size=(m, m)) < 0.6).astype(np.float64)
    src = np.sort(np.concatenate([outside, rng.choice(np.setdiff1d(np.arange(n), outside), 38, replace=False)])).astype(np.int32)
    return Scene("n2n01", nd, "n2n", {}, [Tick(src)], force=False, matrix=matrix, dense=None)


# ---- the scenes by name ----------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "lattice3d": ["lattice3d/" + w for w in LATTICE_MODELS],
    "band": ["band/%s/%s" % (o, w) for o in BAND_ORIGINS for w in BAND_MODELS] + ["sum9/" + w for w in SUM9_MODELS],
    "probs": ["probs/" + w for w in PROB_MODELS],
    "shapes": ["shapes/%s/%d/%d" % (m, n, t) for m in SHAPE_MODELS for n, t in SHAPES],
    "parts": ["parts/%s/%s" % (m, w) for m in SHAPE_MODELS for w in PART_NAMES],
    "cells": ["cells/" + w for w in CELLS],
}


def _make(O, name):
    part = name.split("/")
    if part[0] == "lattice3d":
        return lattice3d(O, part[1])
    if part[0] == "band":
        return band(O, part[1], part[2])
    if part[0] == "sum9":
        return sum9(O, part[1])
    if part[0] == "probs":
        return probs(O, part[1])
    if part[0] == "shapes":
        return shapes(O, part[1], int(part[2]), int(part[3]))
    if part[0] == "parts":
        return parts(O, part[1], part[2])
    if part[0] == "cells":
        return cells_small(O, int(part[2])) if part[1] == "small" else cells(O, part[1])
    if part[0] == "culled":
        return culled(O, part[1], int(part[2]))
    assert name == "n2n01", name
    return n2n01(O)


def scene(O, name):
    if ("scene", name) not in _CACHE:
        _CACHE[("scene", name)] = _make(O, name)
    return _CACHE[("scene", name)]


def expected(O, name, k=0):
    """the oracle's result of tick k of the scene: computed once, shared, left unchanged"""
    if ("exp", name, k) not in _CACHE:
        sc = scene(O, name)
        _CACHE[("exp", name, k)] = Expected(O, sc, sc.ticks[k])
    return _CACHE[("exp", name, k)]
