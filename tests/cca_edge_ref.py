"""Scenes and expected values for the branches of the carrier-sense index that uniform scenes never reach (DESIGN.md sections 4.9 - 4.11:
a cell that overflows into the EVERY list, an EVERY list longer than one LDS chunk, sums that use the high word, a tick of more than
1024 candidates, air times that differ per tick with exact span ends, a batch of RM_MAX_BATCH mostly empty ticks, ld_exponent = 0, a
node outside the fp32 frame).  Expected values come from tests/cca_ref.py::Chain and tests/energy_ref.py::channel_energy alone; no
engine code is involved.  tests/test_cca_edge_ref.py holds every scene to its conditions, tests/test_gpu_cca_edges.py runs them."""
import numpy as np

import cca_ref as CR
import energy_ref as R

_CACHE = {}
MAX_BATCH = 512          # RM_MAX_BATCH
GRID = 64                # the index is a GRID x GRID grid over the square around the bounding box's centre


class EdgeScene:
    """A list of steps, each a plain or a gated tick with times of its own: step k begins at t_begin[k], samples at t_cca[k], its
    frames start at start[k] and last airs[k].  (The attributes cca_ref.Scene has are here too, so that the helpers of the two
    older GPU suites take an EdgeScene.)"""

    def __init__(self, name, nd, params, threshold):
        self.name, self.nd, self.params, self.threshold = name, nd, params, threshold
        self.t_begin, self.t_cca, self.start, self.airs, self.ticks, self.gated = [], [], [], [], [], []

    def add(self, t_begin, t_cca, start, air, src, gated=True):
        assert t_begin <= t_cca <= start and air >= 0
        src = np.asarray(src, dtype=np.int32)
        real = src[(src >= 0) & (src < self.nd.n)]
        assert len(np.unique(real)) == len(real), "a tick's nodes are distinct"
        for lst, v in ((self.t_begin, t_begin), (self.t_cca, t_cca), (self.start, start), (self.airs, air), (self.ticks, src), (self.gated, gated)):
            lst.append(v)
        return len(self.ticks) - 1

    def times(self, k):
        return self.t_begin[k], self.t_cca[k], self.start[k]

    def model(self, O):
        return O.model(O.MODEL_LOGDIST, **self.params)


class Run:
    """cca_batch_ref.Run with per-step (t_begin, t_cca, start, air): a scene's steps through the oracle chain, computed once and left
    unchanged.  Per step: flags and energy (None for a plain tick), Expected, the frames on the air before (expired for the step's
    t_begin) and after it.  `change`: {step: {"air" / "start": value}} -- a boundary moved, for the conditions of scene "times"."""

    def __init__(self, O, sc, steps=None, threshold=None, change=None):
        chain = CR.Chain(O, sc.nd, sc.model(O))
        thr = sc.threshold if threshold is None else threshold
        n = len(sc.ticks) if steps is None else steps
        self.lists = [np.asarray(s, dtype=np.int32) for s in sc.ticks[:n]]
        self.flags, self.energy, self.exp, self.before, self.onair = [], [], [], [], []
        for k, src in enumerate(self.lists):
            t0, tc, ts = sc.times(k)
            air = sc.airs[k]
            if change and k in change:
                ts, air = change[k].get("start", ts), change[k].get("air", air)
            chain.expire(t0)
            self.before.append(chain.onair.copy())
            if sc.gated[k]:
                f, e, x = chain.gated_tick(t0, src, ts, air, tc, thr)
            else:
                f, e, x = None, None, chain.plain_tick(t0, src, ts, air)
            self.flags.append(f)
            self.energy.append(e)
            self.exp.append(x)
            self.onair.append(chain.onair.copy())


def scene(O, name):
    if ("scene", name) not in _CACHE:
        _CACHE[("scene", name)] = {"hotspot": hotspot, "bigtick": bigtick, "times": times, "sparse512": sparse512, "flat": flat}[name](O)
    return _CACHE[("scene", name)]


def run(O, name):
    if ("run", name) not in _CACHE:
        _CACHE[("run", name)] = Run(O, scene(O, name))
    return _CACHE[("run", name)]


def live(frames, t):
    return frames[(frames["src"] >= 0) & (frames["start_us"] <= t) & (t < frames["start_us"] + frames["air_us"])]


def cell_side(nd):
    """the least a grid cell's side can be: the grid spans twice the largest half-extent of the bounding box"""
    return max(float(np.ptp(nd.x)), float(np.ptp(nd.y)), float(np.ptp(nd.z))) / GRID


def sense(O, sc, frames, t, nodes, q80=False):
    """E5 for `nodes` on their own channels over `frames` at t, against the scene's threshold"""
    return R.channel_energy(O, sc.model(O), sc.nd, frames, t, nodes=np.asarray(nodes, dtype=np.int32), threshold=sc.threshold, q80=q80)


def low_words_carry(O, sc, frames, t, node):
    """Does the 128-bit sum of `node` carry out of its low 64 bits, whatever the order of the terms?  (The low words' sum is exact
    mod 2^64, so the number of carries is the same in every order.)  The terms one frame at a time."""
    terms = [sense(O, sc, frames[k:k + 1], t, [node], q80=True)[3][0] for k in range(len(frames))]
    return (sum(q & ((1 << 64) - 1) for q in terms) >> 64) > 0


def _table(O, x, y, channel=None):
    nd = O.NodeTable(len(x))
    nd.x, nd.y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if channel is not None:
        nd.channel[:] = channel
    return nd


def _nearest(nd, node, taken, same_channel=True):
    """the node nearest to `node` (on its channel) that is not in `taken`"""
    d2 = (nd.x - nd.x[node]) ** 2 + (nd.y - nd.y[node]) ** 2
    if same_channel:
        d2[nd.channel != nd.channel[node]] = np.inf
    d2[list(taken)] = np.inf
    d2[node] = np.inf
    return int(np.argmin(d2))


def _neighbours(nd, nodes, taken, same_channel=True):
    out, taken = [], set(taken)
    for j in nodes:
        k = _nearest(nd, int(j), taken, same_channel)
        out.append(k)
        taken.add(k)
    return np.array(out, dtype=np.int32)


# ---- 1. hotspot ----------------------------------------------------------------------------------------------------------------------
HOT_FIELD, HOT_N, HOT_RING, HOT_SIDE = 3000, 1600, 48, 8.0
HOT_QUERY, HOT_GATE, HOT_BATCH = 3, 3, (4, 10)       # the query runs before step 3 (the lone gated tick); steps 4 .. 9 are the batch


def hotspot(O):
    """3000 field nodes at the usual density on 16 channels, 1600 nodes in a box of 8 m (under half a grid cell: at most 4 cells), a
    ring of 48 nodes 4 - 12 m outside that box.  Steps 0 .. 2 (plain) put 1152 hot-spot frames and 300 field frames on the air for
    the whole run; step 3 is a lone gated tick, steps 4 .. 9 a gated batch, half of whose candidates are hot-spot nodes."""
    field, rng = CR.uniform_nodes(O, HOT_FIELD, 51, channels=16)
    cx, cy = 0.37 * field.x.max(), 0.58 * field.y.max()
    hx, hy = cx + rng.uniform(0, HOT_SIDE, HOT_N), cy + rng.uniform(0, HOT_SIDE, HOT_N)
    ang, rad = rng.uniform(0, 2 * np.pi, HOT_RING), rng.uniform(4.0, 12.0, HOT_RING) + HOT_SIDE * 0.75
    rx, ry = cx + HOT_SIDE / 2 + rad * np.cos(ang), cy + HOT_SIDE / 2 + rad * np.sin(ang)
    ch = np.concatenate([field.channel, 11 + np.arange(HOT_N) % 16, 11 + np.arange(HOT_RING) % 16])
    nd = _table(O, np.concatenate([field.x, hx, rx]), np.concatenate([field.y, hy, ry]), ch)
    sc = EdgeScene("hotspot", nd, {"ld_flags": 1, "ld_sigma_db": 3.0, "ld_seed": 0x407}, -30.0)
    sc.hot = np.arange(HOT_FIELD, HOT_FIELD + HOT_N, dtype=np.int32)
    sc.ring = np.arange(HOT_FIELD + HOT_N, nd.n, dtype=np.int32)
    sc.box = (cx, cy, HOT_SIDE)
    hot = rng.permutation(sc.hot)
    sc.hot_on_air, sc.hot_idle = hot[:1152], hot[1152:]
    fld = rng.permutation(HOT_FIELD).astype(np.int32)
    for k in range(3):
        src = np.concatenate([sc.hot_on_air[384 * k:384 * (k + 1)], fld[100 * k:100 * (k + 1)]])
        sc.add(1000 * k, 1000 * k, 1000 * k + 200, 30_000, rng.permutation(src), gated=False)
    idle_field = fld[300:]
    d = np.hypot(nd.x[idle_field] - cx, nd.y[idle_field] - cy)
    near, far = idle_field[np.argsort(d)[:40]], idle_field[np.argsort(d)[-40:]]
    sc.query_nodes = np.concatenate([rng.choice(sc.hot_idle, 60, replace=False), sc.hot_on_air[:20], sc.ring[:24], near, far,
                                     fld[:16]]).astype(np.int32)
    rng.shuffle(sc.query_nodes)

    def cands(n_field):
        c = np.concatenate([rng.choice(sc.hot_idle, 62, replace=False), rng.choice(sc.hot_on_air, 5, replace=False),
                            rng.choice(sc.ring, 8, replace=False), rng.choice(idle_field, n_field, replace=False)]).astype(np.int32)
        rng.shuffle(c)
        return c

    sc.add(3000, 3128, 3200, CR.AIR, cands(75))
    for k in range(4, 10):
        src = cands(75)
        if k == 5:
            src[[3, 77]] = -1
        sc.add(1000 * k, 1000 * k + 128, 1000 * k + 200, CR.AIR, src)
    return sc


# ---- 2. bigtick ----------------------------------------------------------------------------------------------------------------------
BIG_SIZES = (1300, 40, 1100, 40)


def bigtick(O):
    """8000 nodes on 16 channels; step 0 (plain) puts 600 frames on the air, steps 1 .. 4 are ONE batch of overlapping ticks with 1300,
    40, 1100 and 40 candidates.  The short ticks' candidates are the co-channel neighbours of the long ticks' candidates at slots
    >= 1024: what they sense hangs on kept bits beyond the first pass of a 1024-thread workgroup."""
    nd, rng = CR.uniform_nodes(O, 8000, 53, channels=16)
    sc = EdgeScene("bigtick", nd, {"ld_flags": 1, "ld_sigma_db": 3.0, "ld_seed": 0xB16}, -95.0)
    order = rng.permutation(nd.n).astype(np.int32)
    sc.add(0, 0, 200, 30_000, order[:600], gated=False)
    taken = set(order[:600].tolist())
    at = 600
    for b, size in enumerate(BIG_SIZES):
        k = b + 1
        if size > 1024:
            src = order[at:at + size].copy()
            at += size
            taken.update(src.tolist())
            if b == 0:
                src[[5, 500, 1030, 1290]] = -1           # padding at slots below and above 1024
        else:
            high = sc.ticks[-1][1024:]
            src = _neighbours(nd, high[high >= 0][:size], taken)
            taken.update(src.tolist())
        sc.add(1000 * k, 1000 * k + 128, 1000 * k + 200, CR.AIR, src)
    return sc


# ---- 3. times ------------------------------------------------------------------------------------------------------------------------
# (t_begin, t_cca, start, air) of the window's plain tick and of the six ticks of the batch
TIMES = [(0, 0, 100, 3999),         # P: on the air until 4099 -- live at tick 3's sample (4098), gone at tick 4's (4099)
         (1000, 1100, 1200, 3000),  # 0: until 4200 = tick 5's sample: must not count there
         (2000, 2100, 2100, 1500),  # 1
         (2000, 2100, 2100, 2000),  # 2: the times of tick 1, sample == start: tick 1's kept frames are live; until 4100 = tick 4's sample + 1
         (3000, 4098, 4150, 0),     # 3: air 0: never on the air
         (4000, 4099, 4300, 700),   # 4
         (4100, 4200, 4400, 900)]   # 5
# the four boundaries, each moved by 1 us: (what, {step: change}, the step whose flags must change)
TIMES_MOVES = [("tick 0's span ends at tick 5's sample (exclusive end)", {1: {"air": 3001}}, 6),
               ("tick 2's span ends one past tick 4's sample", {3: {"air": 1999}}, 5),
               ("tick 1 starts at tick 2's sample (inclusive start)", {2: {"start": 2101}}, 3),
               ("the window frame ends at tick 4's sample", {0: {"air": 4000}}, 5),
               ("the window frame ends one past tick 3's sample", {0: {"air": 3998}}, 4)]


def times(O):
    """2000 nodes, one channel.  Every later tick's candidates are the neighbours of the nodes whose frames' boundaries it tests."""
    nd, rng = CR.uniform_nodes(O, 2000, 57)
    sc = EdgeScene("times", nd, {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 0x71}, -88.0)
    order = rng.permutation(nd.n).astype(np.int32)
    lists = [order[:60], order[60:120], order[120:180]]
    taken = set(order[:205].tolist())

    def nb(nodes):
        out = _neighbours(nd, nodes, taken)
        taken.update(out.tolist())
        return out

    lists.append(np.concatenate([nb(lists[2][:45]), order[180:195]]))        # tick 2: next to tick 1's
    lists.append(nb(lists[0][:40]))                                          # tick 3: next to the window's
    lists.append(np.concatenate([nb(lists[0][:40]), nb(lists[3][:40])]))     # tick 4: next to the window's and to tick 2's
    lists.append(np.concatenate([nb(lists[1][:50]), order[195:205]]))        # tick 5: next to tick 0's
    for k, (tb, tc, ts, air) in enumerate(TIMES):
        sc.add(tb, tc, ts, air, lists[k], gated=k > 0)
    return sc


# ---- 4. sparse512 --------------------------------------------------------------------------------------------------------------------
SPARSE_FULL = (3, 4, 5, 7, 108, 109, 110, 112, 113, 200, 201, 203, 300, 301, 302, 400, 401, 403, 507, 508, 509)


def sparse512(O):
    """RM_MAX_BATCH ticks of 1000 us, 21 of them with 3 .. 40 candidates, frames of 4500 us; the rest have n_src = 0 -- the first three,
    ticks 8 .. 107, the last two."""
    nd, rng = CR.uniform_nodes(O, 600, 59)
    sc = EdgeScene("sparse512", nd, {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 0x512}, -88.0)
    sizes = dict(zip(SPARSE_FULL, [40, 3, 25, 31, 40, 17, 3, 36, 22, 40, 9, 28, 33, 40, 5, 38, 12, 27, 40, 19, 7]))
    for k in range(MAX_BATCH):
        src = rng.choice(nd.n, sizes[k], replace=False).astype(np.int32) if k in sizes else np.zeros(0, dtype=np.int32)
        if k == 112:
            src[4] = -1
        sc.add(1000 * k, 1000 * k + 128, 1000 * k + 200, 4500, src)
    return sc


# ---- 5. flat -------------------------------------------------------------------------------------------------------------------------
FLAT_QUERY, FLAT_GATE, FLAT_BATCH = 3, 3, (4, 7)


def flat(O):
    """ld_exponent = 0: distance does not matter, every frame's cut-off is infinite or it reaches the floor nowhere.  400 nodes on 4
    channels (half of the nodes on 11, none of channel 14's above the floor), txpower - pl0 = -40 dBm (above the interference floor
    of -110 dBm) for every other node of channels 11 .. 13 and -120 dBm for the rest.  Steps 0 .. 2 (plain) put 300 frames on the air."""
    nd, rng = CR.uniform_nodes(O, 400, 61)
    nd.channel[:] = 11 + rng.choice(4, nd.n, p=[0.5, 0.3, 0.15, 0.05])
    strong = (np.arange(nd.n) % 2 == 0) & (nd.channel != 14)
    nd.txpower[:] = np.where(strong, 0.0, -80.0)
    sc = EdgeScene("flat", nd, {"ld_flags": 1, "ld_exponent": 0.0, "ld_sigma_db": 3.0, "ld_seed": 0xF1A7}, -23.0)
    order = rng.permutation(nd.n).astype(np.int32)
    for k in range(3):
        sc.add(1000 * k, 1000 * k, 1000 * k + 200, 30_000, order[100 * k:100 * (k + 1)], gated=False)
    sc.idle = order[300:]
    sc.query_nodes = rng.permutation(nd.n).astype(np.int32)[:250]
    for k in range(3, 7):
        src = np.concatenate([rng.choice(sc.idle, 30, replace=False), rng.choice(order[:300], 6, replace=False)]).astype(np.int32)
        sc.add(1000 * k, 1000 * k + 128, 1000 * k + 200, CR.AIR, rng.permutation(src))
    return sc


# ---- 6. a node outside the fp32 frame ------------------------------------------------------------------------------------------------
def far_scene(O):
    """tests/test_energy_ref.py's reference scene with one node that sends nothing moved 3 000 km away -> (nd, params, srcs, frames, far)"""
    from test_energy_ref import reference_scene
    nd, params, srcs, _ = reference_scene(O)
    far = int(np.setdiff1d(np.arange(nd.n), srcs)[1234])
    nd.x[far], nd.y[far] = nd.x[far] + 3.0e6, nd.y[far] - 2.0e6
    from radio_sim_amd import workload as W
    return nd, params, srcs, nd.packets(srcs, 0, W.AIR_US), far
