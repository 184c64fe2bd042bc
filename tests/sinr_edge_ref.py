"""Scenes and expected values for the branches of the SINR verdict paths that uniform scenes never reach (DESIGN.md sections 4.4, 4.5
and 6, E3 / E4): sums that carry into the high word, Q80 terms of zero, thresholds met exactly, half duplex with and without air
time, channels that share a bit of the 32-bit channel masks, tables of one to three nodes, time spans that abut, and a chain of
overlapping ticks with every air time around the tick length.  Expected values come from the oracle alone (O.tick over the frames
on the air with first_new, as tests/test_gpu_overlap.py::Replay does); no engine code is involved.  tests/test_sinr_edge_ref.py
holds every scene to its conditions, tests/test_gpu_sinr_edges.py runs them."""
import ctypes as C

import numpy as np

import energy_ref as R

_CACHE = {}
TICK = 1000
LOW = (1 << 64) - 1


class Tick:
    """Either a source list with one start and one air time (src, start, air), or records with times, power and channel of their own."""

    def __init__(self, t_begin, src=None, start=None, air=None, recs=None):
        self.t_begin, self.t_end = t_begin, t_begin + TICK
        self.recs = recs
        if recs is None:
            self.src = np.asarray(src, dtype=np.int32)
            assert len(np.unique(self.src)) == len(self.src), "a tick's nodes are distinct"
            self.start, self.air = t_begin if start is None else start, air
        else:
            self.src, self.start, self.air = recs["src"].astype(np.int32), None, None

    def __len__(self):
        return len(self.src)

    def packets(self, nd):
        return self.recs.copy() if self.recs is not None else nd.packets(self.src, self.start, self.air)

    def latest_end(self, nd):
        p = self.packets(nd)
        return int((p["start_us"] + p["air_us"]).max()) if len(p) else self.t_begin


class Scene:
    """A node table, model parameters, ticks in time order, and the sources of one more lone tick (`tail`) that looks at what the
    scene left on the air.  `by_sources`: every tick is a source list; `contained`: no frame but the last tick's outlives its tick."""

    def __init__(self, name, nd, params, ticks, tail, tail_air=320):
        self.name, self.nd, self.params, self.ticks = name, nd, dict(params, ld_flags=1), ticks
        self.tail, self.tail_air = np.asarray(tail, dtype=np.int32), tail_air
        self.by_sources = all(t.recs is None for t in ticks)
        self.contained = all(t.latest_end(nd) <= t.t_end for t in ticks[:-1])
        assert nd.n <= 300 and len(ticks) <= 20
        assert all(a.t_end <= b.t_begin for a, b in zip(ticks, ticks[1:]))

    def model(self, O):
        return O.model(O.MODEL_LOGDIST, **self.params)

    def end(self):
        """the earliest begin of the tail tick: the last tick's end"""
        return self.ticks[-1].t_end


def _live(frames, t_begin):
    return frames[frames["start_us"] + frames["air_us"] > t_begin]       # E4


class Run:
    """A scene's ticks through the oracle, computed once and left unchanged: per tick the frames on the air before it (expired for
    its t_begin), its packets and the oracle's result for them."""

    def __init__(self, O, sc):
        self.O, self.sc, self.mdl = O, sc, sc.model(O)
        self.before, self.new, self.exp = [], [], []
        onair = np.zeros(0, dtype=O.PACKET_DTYPE)
        for tk in sc.ticks:
            onair = _live(onair, tk.t_begin)
            new = tk.packets(sc.nd)
            self.before.append(onair)
            self.new.append(new)
            self.exp.append(O.tick(self.mdl, sc.nd, np.concatenate([onair, new]), first_new=len(onair)))
            onair = np.concatenate([onair, new])
        self.onair = onair
        self._tails = {}

    def tail(self, t_begin):
        """(packets, the oracle's result, frames still on the air) of the tail tick at t_begin"""
        key = t_begin
        if key not in self._tails:
            sc = self.sc
            onair = _live(self.onair, t_begin)
            new = sc.nd.packets(sc.tail, t_begin, sc.tail_air)
            self._tails[key] = (new, self.O.tick(self.mdl, sc.nd, np.concatenate([onair, new]), first_new=len(onair)), len(onair))
        return self._tails[key]

    def alone(self, k):
        """tick k's packets with nothing else on the air"""
        return self.O.tick(self.mdl, self.sc.nd, self.new[k])


def offsets(res, n_new):
    """pkt_offset as the engine returns it, from the oracle's packet column"""
    return np.searchsorted(res.pkt, np.arange(n_new + 1)).astype(np.uint32)


def rssi_of(O, sc, frame, node):
    """E1 / E2 of one frame (a PACKET_DTYPE array of length 1) at `node`"""
    mdl, ns = sc.model(O), sc.nd.as_struct()
    return O.lib().orc_logdist_rssi(C.byref(mdl), C.cast(frame.ctypes.data, C.POINTER(O.Packet)), C.byref(ns), int(node))


def q80_terms(O, sc, frames, node, channel):
    """the Q80 term of every frame of `frames` (all taken as on the air) that counts at `node` on `channel`, one frame at a time
    -> list of Python integers (a frame below the interference floor, on another channel or sent by `node` gives no term)"""
    out = []
    for k in range(len(frames)):
        f = frames[k:k + 1].copy()
        f["start_us"], f["air_us"] = 0, 1
        _, _, cnt, q = R.channel_energy(O, sc.model(O), sc.nd, f, 0, nodes=np.array([node], dtype=np.int32), channel=int(channel), q80=True)
        if cnt[0]:
            out.append(q[0])
    return out


def low_word_carries(terms):
    """how often the 128-bit sum of `terms` carries out of its low 64 bits (the same in every order), and its high word"""
    return sum(q & LOW for q in terms) >> 64, sum(terms) >> 64


def _field(O, n, side, seed, channels=None):
    rng = np.random.default_rng(seed)
    nd = O.NodeTable(n)
    nd.x, nd.y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    if channels is not None:
        nd.channel[:] = rng.choice(channels, n)
    return nd, rng


# ---- 1. hot --------------------------------------------------------------------------------------------------------------------------
HOT_CHANNELS = (28, -4, 60)          # all three set bit 28 of a 32-bit channel mask (1u << (ch & 31))


def hot(O):
    """65 nodes in a square of 3 m, pl0 = 0 and d0 = 1: every power is between 0.01 and 1 mW (Q80 terms with both words in use), a
    receiver's sum is a few mW.  Tick 0: every second node, air 320; tick 1: the others, on the air beyond their tick."""
    nd, rng = _field(O, 65, 3.0, 1, channels=HOT_CHANNELS)
    params = {"ld_pl0_db": 0.0, "ld_d0": 1.0, "ld_exponent": 3.0, "ld_ifloor_dbm": -300.0, "ld_capture_db": -10.0}
    ticks = [Tick(0, np.arange(0, 65, 2), air=320), Tick(TICK, rng.permutation(np.arange(1, 65, 2)), air=1500)]
    return Scene("hot", nd, params, ticks, tail=[0, 7, 20, 33, 64])


# ---- 2. bounds -----------------------------------------------------------------------------------------------------------------------
BOUNDS = ("ifloor", "sensitivity", "capture")
_BOUND_PARAM = {"ifloor": "ld_ifloor_dbm", "sensitivity": "ld_sensitivity_dbm", "capture": "ld_capture_db"}


def _bounds_scene(O, name, extra):
    nd, rng = _field(O, 120, 217.0, 7)
    params = dict({"ld_sigma_db": 4.0, "ld_seed": 0xB0}, **extra)
    order = rng.permutation(nd.n).astype(np.int32)
    ticks = [Tick(0, order[:40], air=320), Tick(TICK, order[40:70], air=1500)]
    return Scene(name, nd, params, ticks, tail=order[70:78])


def bounds_link(O, which):
    """the link of the base run's tick 0 whose own oracle value becomes the threshold -> (position in the result, value)"""
    exp = run(O, "bounds/base").exp[0]
    sc = scene(O, "bounds/base")
    heard_by = np.bincount(exp.dst, minlength=sc.nd.n)
    sending = np.isin(exp.dst, sc.ticks[0].src)
    if which == "ifloor":           # the weakest link at a receiver that hears a second frame of the tick: that frame loses an interferer
        ok = np.flatnonzero((heard_by[exp.dst] >= 2) & ~sending)
        k = int(ok[np.argmin(exp.rssi[ok])])
        return k, float(exp.rssi[k])
    if which == "sensitivity":      # the weakest link: the next double as the sensitivity drops this link alone
        k = int(np.argmin(exp.rssi))
        return k, float(exp.rssi[k])
    ok = np.flatnonzero(exp.verdict == O.DELIVERED)           # the delivered link with the least sinr
    k = int(ok[np.argmin(exp.sinr[ok])])
    return k, float(exp.sinr[k])


def bounds(O, which, step):
    """`which` threshold at the chosen link's own value (step 'exact') or at the next double above it (step 'next')"""
    _, v = bounds_link(O, which)
    v = v if step == "exact" else float(np.nextafter(v, np.inf))
    return _bounds_scene(O, "bounds/%s/%s" % (which, step), {_BOUND_PARAM[which]: v})


# ---- 3. everyone ---------------------------------------------------------------------------------------------------------------------
def everyone(O, n):
    """ld_exponent = 0: no finite cut-off, every node hears every frame.  Tick 0: all nodes, air 320 (every receiver is on the air
    itself); tick 1: all nodes, air 0 (nothing overlaps anything); tick 2: one frame (the sum less the link's own power is 0)."""
    nd, rng = _field(O, n, 100.0, 64 + n)
    params = {"ld_exponent": 0.0, "ld_sigma_db": 3.0, "ld_seed": 5}
    ticks = [Tick(0, rng.permutation(n), air=320), Tick(TICK, rng.permutation(n), air=0), Tick(2 * TICK, [n // 2], air=1500)]
    return Scene("everyone/%d" % n, nd, params, ticks, tail=[0, 1, n // 2, n - 1])


# ---- 4. quiet ------------------------------------------------------------------------------------------------------------------------
QUIET = {"clip0": {"ld_sigma_db": 12.0, "ld_clip": 0.0, "ld_seed": 3}, "clip1": {"ld_sigma_db": 12.0, "ld_clip": 1.0, "ld_seed": 3},
         "coincident": {"ld_d0": 30.0}, "noise60": {"ld_noise_dbm": -60.0}}


def quiet(O, variant):
    """txpower -300 dBm, sensitivity and interference floor -450 dBm: every link is heard, every frame is an interferer at every node
    and every linear power (below 1e-34 mW) is a Q80 term of zero: sinr = rssi - noise.  The capture threshold lies inside the range
    of those values, so both verdicts occur."""
    nd, rng = _field(O, 70, 60.0, 9)
    nd.txpower[:] = -300.0
    if variant == "coincident":
        nd.x[:], nd.y[:] = 5.0, -3.0
    params = dict({"ld_sensitivity_dbm": -450.0, "ld_ifloor_dbm": -450.0, "ld_capture_db": -270.0 - (40.0 if variant == "noise60" else 0.0)},
                  **QUIET[variant])
    if variant == "coincident":
        params["ld_capture_db"] = -240.0          # every rssi is -340 exactly: sinr == capture on every link
    order = rng.permutation(nd.n).astype(np.int32)
    ticks = [Tick(0, order[:35], air=320), Tick(TICK, order[35:55], air=1500)]
    return Scene("quiet/" + variant, nd, params, ticks, tail=order[55:60])


# ---- 5. tiny -------------------------------------------------------------------------------------------------------------------------
def tiny(O, what):
    none = np.zeros(0, dtype=np.int32)
    if what == "1":
        nd = O.NodeTable(1)
        ticks = [Tick(0, [0], air=320), Tick(TICK, none, air=320), Tick(2 * TICK, [0], air=1500)]
        tail = [0]
    elif what == "2":
        nd = O.NodeTable(2)
        nd.x[1] = 10.0
        ticks = [Tick(0, [0, 1], air=320), Tick(TICK, [1], air=0), Tick(2 * TICK, [0], air=1500)]
        tail = [1]
    elif what == "3":       # node 2 on a channel of its own: its frame has no receiver, and it hears nobody
        nd = O.NodeTable(3)
        nd.x[:], nd.y[:] = [0.0, 8.0, 3.0], [0.0, 0.0, 4.0]
        nd.channel[2] = 11
        ticks = [Tick(0, [2, 0, 1], air=320), Tick(TICK, [2], air=1000), Tick(2 * TICK, none, air=320), Tick(3 * TICK, [1, 0], air=1500)]
        tail = [2, 0]
    else:                   # a batch of only empty ticks
        nd = O.NodeTable(3)
        nd.x[:] = [0.0, 8.0, 3.0]
        ticks = [Tick(k * TICK, none, air=320) for k in range(3)]
        tail = [1, 2]
    return Scene("tiny/" + what, nd, {}, ticks, tail)


# ---- 6. spans ------------------------------------------------------------------------------------------------------------------------
# (name, start, air): one tick of 1000 us, every frame ends by its end
SPANS = [("zero_at_begin", 0, 0),            # air 0 at the tick's begin: overlaps nothing (the oracle's strict inequalities)
         ("twin_a", 100, 300), ("twin_b", 100, 300),      # two identical spans
         ("near", 300, 200),                 # its source is the nearest node to twin_a's and the spans overlap: half duplex both ways
         ("later", 600, 100),                # its source is in twin_a's reach, the spans do not overlap: no half duplex
         ("abut_a", 450, 150), ("abut_b", 600, 200),      # one ends at 600, the other starts at 600
         ("lap_a", 700, 151), ("lap_b", 850, 150),        # the same, overlapping by 1 us
         ("outer", 50, 900), ("inner", 450, 50),          # a span inside another
         ("zero_inside", 250, 0)]            # air 0 strictly inside other spans: start < end and end > start hold -- it interferes
SPANS_MOVED = "abut_b"                       # the second variant: this frame starts 1 us earlier


def spans(O, moved):
    nd, rng = _field(O, 90, 150.0, 11)
    nd.channel[::9] = 11
    a = 40
    d = np.hypot(nd.x - nd.x[a], nd.y - nd.y[a])
    d[nd.channel != 26] = np.inf
    near = np.argsort(d)[:len(SPANS)].astype(np.int32)         # near[0] == a; the frames' sources: the nodes closest to it
    who = dict(zip(["twin_a", "near", "later"] + [s[0] for s in SPANS if s[0] not in ("twin_a", "near", "later")], near.tolist()))
    recs = nd.packets(np.array([who[s[0]] for s in SPANS], dtype=np.int32), 0, 0)
    for k, (name, start, air) in enumerate(SPANS):
        recs["start_us"][k], recs["air_us"][k] = start - (1 if moved and name == SPANS_MOVED else 0), air
        if name == "twin_b":
            recs["txpower"][k] = 5.5         # not the table's
        if name == "outer":
            recs["txpower"][k] = -7.0
        if name == "inner":
            recs["channel"][k] = 11          # sent on a channel its node does not listen on
    sc = Scene("spans/" + ("moved" if moved else "base"), nd, {"ld_sigma_db": 3.0, "ld_seed": 0x5A}, [Tick(0, recs=recs)], tail=[int(near[0]), 3])
    sc.who = who
    return sc


# ---- 7. chain ------------------------------------------------------------------------------------------------------------------------
CHAIN_SIZES = [0, 1, 64, 65, 0, 130, 257, 3, 40, 0, 129, 1, 200, 63, 0, 100, 17]
CHAIN_AIRS = [300, 20000, 1000, 999, 1001, 1001, 1001, 0, 8128, 1000, 300, 20000, 999, 8128, 0, 1000, 8128]
CHAIN_CUTS = (3, 7, 12)                      # the chain as two batches: ticks [0, cut) and [cut, 17)


CHAIN_OFFSETS = {15: 250, 16: 250}           # frames that start this long after their tick begins (the others: with it)
# ticks with air 1000 before a tick that has frames: they end exactly where those start -- tick 2's at tick 3's begin (gone by E4
# as well), tick 15's 250 us into tick 16 (still on the air when it begins, and no overlap)
CHAIN_ENDS_AT_NEXT = (2, 15)


def chain(O, airs=None):
    """257 nodes on three channels, shadowing on; 17 ticks of 1000 us whose frames stay on the air for 0 us to 20 ticks.  Tick 6 is
    the whole table, on the air 1 us into tick 7: every receiver of tick 7's frames (air 0) is on the air itself.  `airs`: other
    air times over the same nodes and sources (the conditions of tests/test_sinr_edge_ref.py move one by 1 us)."""
    nd, rng = _field(O, 257, 50.0 * np.sqrt(np.pi * 257 / 30.0), 17, channels=[11, 12, 13])
    ticks = [Tick(k * TICK, rng.choice(nd.n, s, replace=False), start=k * TICK + CHAIN_OFFSETS.get(k, 0), air=a)
             for k, (s, a) in enumerate(zip(CHAIN_SIZES, airs or CHAIN_AIRS))]
    return Scene("chain", nd, {"ld_sigma_db": 4.0, "ld_seed": 0xC4A1}, ticks, tail=rng.choice(nd.n, 30, replace=False))


# ---- the scenes by name --------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "hot": ["hot"],
    "bounds": ["bounds/%s/%s" % (w, s) for w in BOUNDS for s in ("exact", "next")],
    "everyone": ["everyone/64", "everyone/65"],
    "quiet": ["quiet/" + v for v in QUIET],
    "tiny": ["tiny/1", "tiny/2", "tiny/3", "tiny/empty"],
    "spans": ["spans/base", "spans/moved"],
    "chain": ["chain"],
}


def _make(O, name):
    part = name.split("/")
    if part[0] == "hot":
        return hot(O)
    if part[0] == "bounds":
        return _bounds_scene(O, name, {}) if part[1] == "base" else bounds(O, part[1], part[2])
    if part[0] == "everyone":
        return everyone(O, int(part[1]))
    if part[0] == "quiet":
        return quiet(O, part[1])
    if part[0] == "tiny":
        return tiny(O, part[1])
    if part[0] == "spans":
        return spans(O, part[1] == "moved")
    assert name == "chain", name
    return chain(O)


def scene(O, name):
    if ("scene", name) not in _CACHE:
        _CACHE[("scene", name)] = _make(O, name)
    return _CACHE[("scene", name)]


def run(O, name):
    if ("run", name) not in _CACHE:
        _CACHE[("run", name)] = Run(O, scene(O, name))
    return _CACHE[("run", name)]
