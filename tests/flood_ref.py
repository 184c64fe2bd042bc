"""Reference of the dissemination floods: a plain-Python state machine written from the rules alone --
Python integers per node --, and the scenes the CPU and GPU tiers play.  No engine code is involved.  A scene is a function of a
DRIVER: the driver owns the reference state, evaluates ticks (the CPU tier: by the oracle; the GPU tier: by the engine, whose
copied-out result then advances the reference) and may compare after every step.  tests/test_flood_ref.py holds the scenes'
conditions for the reference alone, so that no GPU test passes vacuously."""
import numpy as np

from oracle import oracle as O

import cca_ref
import listen_ref as LR
import neighbors_ref as N
import traffic_ref as T

DELIVERED = 2          # rm_verdict
M64 = (1 << 64) - 1
NODE_FIELDS = ("first_us", "start_us", "fire_us", "rssi_bits", "parent", "hop", "interval", "c", "sent", "suppressed", "heard", "deferred")
TOTALS = ("covered", "seeds", "sent", "suppressed", "heard", "deferred", "stray", "skipped_slots", "max_hop", "last_first_us")
DEFAULTS = dict(imin_us=8000, doublings=4, max_intervals=8, redundancy=2, max_hops=255, seed=0)


def valid(p):
    return (2 <= p["imin_us"] <= 1 << 32 and 0 <= p["doublings"] <= 16 and 1 <= p["max_intervals"] <= 64 and 0 <= p["redundancy"] <= 255
            and 1 <= p["max_hops"] <= 65535)


def fire(p, node, first_us, m):
    """-> (start_us, fire_us) of interval m of a node that got the data at first_us; m == max_intervals: (-1, -1)"""
    if m >= p["max_intervals"]:
        return -1, -1
    length = lambda i: p["imin_us"] << min(i, p["doublings"])
    start = first_us + sum(length(i) for i in range(m))
    half = length(m) // 2
    h = T.mix64(T.mix64(T.mix64((p["seed"] + T.GOLDEN) & M64) ^ (node & 0xFFFFFFFF)) ^ (first_us & M64))
    h = T.mix64(h ^ m)
    return start, start + half + ((h * half) >> 64)


class Result:
    """one slot's result as the advance reads it: the tx records' src / start / air per packet number, pkt_offset, dst, verdict and
    the bits of rssi per link"""

    def __init__(self, src, start, air, pkt_offset, dst, verdict, rssi, lost=False):
        self.src = [int(v) for v in src]
        n = len(self.src)
        self.start = [int(start)] * n if np.isscalar(start) else [int(v) for v in start]
        self.air = [int(air)] * n if np.isscalar(air) else [int(v) for v in air]
        self.pkt_offset = [int(v) for v in pkt_offset]
        self.dst = [int(v) for v in dst]
        self.verdict = [int(v) for v in verdict]
        self.rssi_bits = [int(v) for v in np.ascontiguousarray(rssi, dtype=np.float64).view(np.uint64)]
        self.lost = bool(lost)
        assert len(self.pkt_offset) == n + 1


def records_result(n_nodes, src, start, air, pkt_offset, dst, verdict, rssi, lost=False):
    """a tick over a source list: the record of an entry outside the table -- padding, or a candidate the gate deferred -- has
    src -1 and air_us 0 (what the device ticks write for such a slot), every other one the tick's air time"""
    s = np.asarray(src, dtype=np.int64)
    ok = (s >= 0) & (s < n_nodes)
    return Result(np.where(ok, s, -1), [int(start)] * len(s), np.where(ok, int(air), 0), pkt_offset, dst, verdict, rssi, lost)


class State:
    def __init__(self, n, **params):
        self.p = dict(DEFAULTS, **params)
        assert valid(self.p)
        self.n = n
        self.clear()

    def clear(self):
        n = self.n
        self.first, self.start, self.fire = [-1] * n, [-1] * n, [-1] * n
        self.rssi_bits, self.parent, self.hop = [0] * n, [-1] * n, [-1] * n
        self.m, self.c = [0] * n, [0] * n
        self.cnt = {f: [0] * n for f in ("sent", "suppressed", "heard", "deferred")}
        self.t = {f: 0 for f in ("seeds", "stray", "skipped_slots", "receptions")}

    # ---- the rules' words
    def has(self, j):
        return self.first[j] >= 0

    def due(self, j, t):
        return self.has(j) and self.m[j] < self.p["max_intervals"] and self.fire[j] <= t

    def _schedule(self, j):
        self.start[j], self.fire[j] = fire(self.p, j, self.first[j], self.m[j])

    def _get(self, j, t, parent, hop, rssi_bits):
        self.first[j], self.parent[j], self.hop[j], self.rssi_bits[j], self.m[j], self.c[j] = t, parent, hop, rssi_bits, 0, 0
        self._schedule(j)

    def _next_interval(self, j):
        self.m[j] += 1
        self.c[j] = 0
        self._schedule(j)

    # ---- the calls
    def seed(self, nodes, time_us):
        for j in nodes:
            j = int(j)
            if 0 <= j < self.n and not self.has(j):
                self._get(j, time_us, -1, 0, 0)
                self.t["seeds"] += 1

    def sources(self, time_us, cap):
        k, lst = self.p["redundancy"], []
        for j in range(self.n):
            if not self.due(j, time_us):
                continue
            if k > 0 and self.c[j] >= k:
                self.cnt["suppressed"][j] += 1
                self._next_interval(j)
            else:
                lst.append(j)
        return (lst + [-1] * cap)[:cap], len(lst)

    def advance(self, res, cand=None):
        """one slot's result; cand: the candidate list handed to the evaluating call, or None"""
        if res.lost:
            self.t["skipped_slots"] += 1
            return
        n_new = len(res.src)
        P = n_new if cand is None else min(len(cand), n_new)
        seen, senders, deferred = set(), [], []
        for p in range(P):
            j = int(res.src[p] if cand is None else cand[p])
            if not 0 <= j < self.n or not self.has(j):
                continue
            if j in seen or not self.due(j, res.start[p]):
                seen.add(j)
                self.t["stray"] += 1
                continue
            seen.add(j)
            (deferred if res.src[p] != j else senders).append(j)
        sending = set(senders)
        c_inc, best = {}, {}
        for p in range(n_new):
            s = res.src[p]
            if not 0 <= s < self.n or not self.has(s):
                continue
            t_end = res.start[p] + res.air[p]
            for i in range(res.pkt_offset[p], res.pkt_offset[p + 1]):
                d = res.dst[i]
                if res.verdict[i] != DELIVERED or not 0 <= d < self.n:
                    continue
                self.cnt["heard"][d] += 1
                if self.has(d):
                    if d not in sending and t_end >= self.start[d]:
                        c_inc[d] = c_inc.get(d, 0) + 1
                elif self.hop[s] + 1 <= self.p["max_hops"]:
                    if d not in best or (t_end, p) < best[d][0]:
                        best[d] = ((t_end, p), s, self.hop[s] + 1, res.rssi_bits[i])
        for j in deferred:
            self.cnt["deferred"][j] += 1
        for j in senders:
            self.cnt["sent"][j] += 1
            self._next_interval(j)
        for d, k in c_inc.items():
            self.c[d] += k
        for d, ((t_end, _), s, hop, rb) in best.items():
            self._get(d, t_end, s, hop, rb)
            self.t["receptions"] += 1

    # ---- what the reads return
    def totals(self):
        covered = [j for j in range(self.n) if self.has(j)]
        t = {f: sum(self.cnt[f]) for f in self.cnt}
        t.update(covered=len(covered), seeds=self.t["seeds"], stray=self.t["stray"], skipped_slots=self.t["skipped_slots"],
                 max_hop=max([self.hop[j] for j in covered], default=0), last_first_us=max([self.first[j] for j in covered], default=0))
        return t

    def table(self):
        out = {f: list(self.cnt[f]) for f in self.cnt}
        out.update(first_us=list(self.first), start_us=list(self.start), fire_us=list(self.fire), rssi_bits=list(self.rssi_bits),
                   parent=list(self.parent), hop=list(self.hop), interval=list(self.m), c=list(self.c))
        return out

    def check(self):
        """the identities"""
        t = self.totals()
        assert t["covered"] == self.t["seeds"] + self.t["receptions"], t
        for j in range(self.n):
            assert self.m[j] == self.cnt["sent"][j] + self.cnt["suppressed"][j], j
            assert self.has(j) or (self.parent[j], self.hop[j], self.m[j], self.start[j], self.fire[j]) == (-1, -1, 0, -1, -1), j
            assert (self.fire[j] == -1) == (not self.has(j) or self.m[j] == self.p["max_intervals"]), j


# ---- drivers ---------------------------------------------------------------------------------------------------------------------

KIND = {"null": 0, "udgm": 1, "logdist": 4}
TICK, AIR = 5000, 4256
UDGM = {"udgm_transmission_range": 50.0, "udgm_interference_range": 100.0}


class Driver:
    """the CPU tier's driver: the reference state over ticks the oracle evaluates.  The GPU tier subclasses it
    (tests/test_gpu_flood.py): every call also goes to the engine, ticks are the engine's, and the two states are compared after
    every step.  listen: E13's schedule table (one (period, on, phase) per node) or None"""

    def __init__(self, nd, kind, params, listen=None, **flood):
        self.nd, self.kind, self.params, self.listen = nd, kind, dict(params), listen
        self.ref = State(nd.n, **flood)
        self.chain = None
        self.capacity = None
        self.log = {"truncated": 0, "steps": 0, "ties": 0, "collided": 0, "missed": 0, "deferred_lists": 0, "foreign_delivered": 0,
                    "foreign_collided": 0}

    # -- evaluation by the oracle
    def _chain(self):
        if self.chain is None:
            self.chain = cca_ref.Chain(O, self.nd, O.model(KIND[self.kind], **self.params))
        return self.chain

    def _expected(self, src, e, start, air):
        verdict = e.verdict
        if self.listen is not None and e.raw is not None:
            verdict, _ = LR.apply(e.new, e.raw, self.listen)
        lost = self.capacity is not None and e.count > self.capacity
        return self.watch(records_result(self.nd.n, src, start, air, e.pkt_offset, e.dst, verdict, e.rssi, lost), e.verdict)

    def watch(self, res, before=None):
        """what the scenes' conditions count: first receptions decided by the tie-break, collided and missed copies, foreign frames"""
        ref, at = self.ref, {}
        for p, s in enumerate(res.src):
            for i in range(res.pkt_offset[p], res.pkt_offset[p + 1]):
                if not 0 <= s < ref.n:
                    continue
                if not ref.has(s):
                    self.log["foreign_delivered"] += res.verdict[i] == DELIVERED
                    continue
                if res.verdict[i] == DELIVERED and not ref.has(res.dst[i]):
                    at[res.dst[i]] = at.get(res.dst[i], 0) + 1
                if res.verdict[i] != DELIVERED:
                    self.log["collided"] += 1
                    self.log["foreign_collided"] += any(0 <= q < ref.n and not ref.has(q) for q in res.src)
                if before is not None and int(before[i]) == DELIVERED and res.verdict[i] != DELIVERED:
                    self.log["missed"] += 1
        self.log["ties"] += sum(1 for v in at.values() if v > 1)
        return res

    def set_capacity(self, cap):
        """the context's link capacity: a tick with more heard links is lost"""
        self.capacity = cap

    def tick(self, t_begin, t_end, src, start, air):
        """a plain lone tick over the source list (padding: outside the table) -> Result"""
        return self._expected(src, self._chain().plain_tick(t_begin, src, start, air), start, air)

    def tick_cca(self, t_begin, t_end, src, start, air, cca_time, threshold):
        """a gated lone tick -> Result (a deferred candidate's record has src -1)"""
        flags, _, e = self._chain().gated_tick(t_begin, src, start, air, cca_time, threshold)
        return self._expected(np.where(flags != 0, -1, np.asarray(src, dtype=np.int32)), e, start, air)

    def batch(self, t_begin, t_end, lists, starts, air):
        """a batch of self-contained ticks: one after the other"""
        return [self.tick(t_begin[b], t_end[b], lists[b], starts[b], air) for b in range(len(lists))]

    # -- the feature's calls
    def seed(self, nodes, time_us):
        self.ref.seed(nodes, time_us)
        self.after("seed")

    def sources(self, time_us, cap):
        lst, count = self.ref.sources(time_us, cap)
        if count > cap:
            self.log["truncated"] += 1
        self.after("sources")
        return lst, count

    def advance(self, res, cand=None, slot=0):
        self.ref.advance(res, cand)
        self.log["steps"] += 1
        self.after("advance")

    def reset(self):
        self.ref.clear()
        self.after("reset")

    def after(self, what):
        self.ref.check()


def next_time(d, t, tick, at=100):
    """the start of the first tick not before t in which a node is due `at` us into it, None: nobody fires any more"""
    fires = [f for j, f in enumerate(d.ref.fire) if f >= 0]
    return None if not fires else max(t, -(-(min(fires) - at) // tick) * tick)


def run_steps(d, n_steps, cap, t0=0, tick=TICK, air=AIR, skip=True, stop=None, foreign=None):
    """a step at t: the due nodes' list at t + 100 (and the foreign sources of foreign(t)), a lone tick of it, the advance.  skip: ticks
    in which nobody is due are left out.  stop(d): ends the run -> the time of the next step"""
    t = t0
    for _ in range(n_steps):
        if skip:
            t = next_time(d, t, tick)
            if t is None:
                break
        lst, count = d.sources(t + 100, cap)
        if foreign is not None:
            lst = lst + foreign(t)
        d.advance(d.tick(t, t + tick, lst, t + 100, air))
        t += tick
        if stop is not None and stop(d):
            break
    return t


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

def line_nodes(n, pitch=40.0):
    """n nodes in a row `pitch` m apart: under UDGM 50 / 100 at 40 m node i's frame reaches i - 1 and i + 1"""
    nd = O.NodeTable(n)
    nd.x = pitch * np.arange(n)
    return nd


LINE = dict(imin_us=2 * TICK, doublings=2, max_intervals=12, redundancy=0, max_hops=255, seed=7)


def scene_line(make, n):
    """one seed at an end: the data moves a hop at a time, every node's hop is its distance"""
    d = make(line_nodes(n), "udgm", UDGM, **LINE)
    d.seed([0], 0)
    run_steps(d, 40 * n, n, stop=lambda d: d.ref.totals()["covered"] == n)
    return d


def clique_nodes(n):
    """n nodes on a disc of 15 m: under UDGM 50 / 100 everybody hears everybody"""
    nd = O.NodeTable(n)
    rng = np.random.default_rng(n)
    r, a = 15.0 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    nd.x, nd.y = r * np.cos(a), r * np.sin(a)
    return nd


CLIQUE_TICK, CLIQUE_AIR = 1000, 512


def scene_clique(make, n, k, intervals=3):
    """the seed's frame covers everybody; then the first lone sender of an interval silences the rest (k = 1) or nobody is (k = 0)"""
    d = make(clique_nodes(n), "udgm", UDGM, imin_us=1 << 18, doublings=1, max_intervals=intervals, redundancy=k, seed=n)
    d.seed([0], 0)
    t = run_steps(d, 1, n, tick=CLIQUE_TICK, air=CLIQUE_AIR)
    d.covered_after_first = d.ref.totals()["covered"]
    run_steps(d, 4 * n * intervals, n, t0=t, tick=CLIQUE_TICK, air=CLIQUE_AIR)
    return d


def lattice_nodes(side=9, pitch=50.0):
    """side x side nodes `pitch` apart, txpower 0: under the log-distance defaults (reach 68 m) the four neighbours are heard"""
    nd = O.NodeTable(side * side)
    k = np.arange(side * side)
    nd.x, nd.y = pitch * (k % side), pitch * (k // side)
    nd.txpower = np.zeros(side * side)
    return nd


# capture at -1 dB: two equally strong frames are both received (the tie-break decides), three are not
LATTICE = dict(N.PLAIN, **dict(N.SINR, ld_capture_db=-1.0))
LATTICE_FLOOD = dict(imin_us=4 * TICK, doublings=2, max_intervals=6, redundancy=2, max_hops=255, seed=11)


def lattice_listen(n):
    """E13 for every fifth node: awake 3 ms of every 7 ms"""
    return [(7000, 3000, (131 * j) % 7000) if j % 5 == 2 else (0, 0, 0) for j in range(n)]


def scene_lattice(make, side=33, steps=60):
    """the seed in the middle of side x side nodes on the SINR medium, duty-cycled receivers among them: diagonal neighbours get two
    copies at once, inner nodes collisions"""
    nd = lattice_nodes(side)
    d = make(nd, "logdist", LATTICE, listen=lattice_listen(nd.n), **LATTICE_FLOOD)
    d.seed([nd.n // 2], 0)
    run_steps(d, steps, nd.n)
    return d


def scene_foreign(make, with_foreign=True):
    """a line 50 m apart on the SINR medium whose far half never gets the data (max_hops): nodes there send in every tick all the
    same, and node 6's frames, as strong at node 5 as node 4's, collide with them in three ticks of four"""
    n = 12
    nd = line_nodes(n, 50.0)
    nd.txpower = np.zeros(n)
    d = make(nd, "logdist", dict(N.PLAIN, **N.SINR), **dict(LINE, max_hops=5, max_intervals=6))
    d.seed([0], 0)
    run_steps(d, 120, n + 2, skip=False, foreign=(lambda t: [6, 9] if (t // TICK) % 4 != 1 else [8]) if with_foreign else None)
    return d


GATED_TICK = 1000


def scene_gated(make, cand, steps=160):
    """9 x 9 on the SINR medium, gated ticks of 1 ms whose frames outlive them: a due node that senses a frame is deferred"""
    nd = lattice_nodes()
    d = make(nd, "logdist", LATTICE, **dict(LATTICE_FLOOD, imin_us=8 * GATED_TICK, redundancy=3))
    d.seed([0, 40], 0)
    t = 0
    for _ in range(steps):
        t = next_time(d, t, GATED_TICK, 200)
        if t is None:
            break
        lst, count = d.sources(t + 200, nd.n)
        res = d.tick_cca(t, t + GATED_TICK, lst, t + 200, AIR, t + 128, -88.0)
        if any(s != c for s, c in zip(res.src, lst) if 0 <= c < nd.n):
            d.log["deferred_lists"] += 1
        d.advance(res, lst if cand else None)
        t += GATED_TICK
    return d


def field_nodes(n, seed=3, k=12.0):
    nd, _ = cca_ref.uniform_nodes(O, n, seed, k=k)
    nd.txpower = np.zeros(n)
    return nd


def scene_big(make, n):
    """a random field, every third node a seed (duplicates, padding and entries outside the table in the list): many due at once,
    the list asked with caps below and above the count; then ticks of the first 24"""
    d = make(field_nodes(n), "logdist", N.PLAIN, imin_us=2 * TICK, doublings=1, max_intervals=3, redundancy=1, seed=n)
    seeds = list(range(0, n, 3))
    d.seed(seeds[:5] + [-1, n, n + 7, 0, 3, 3] + seeds[5:], 0)
    asked = [d.sources(TICK - 1, 7)[1]]                 # (before anybody fires)
    m = d.ref.sources(2 * TICK, 1)[1]                   # (k = 1, c = 0: nobody is suppressed, so the walk changes nothing)
    for cap in (m + 1, m, m - 1, 1, n):
        asked.append(d.sources(2 * TICK, cap)[1])
    d.asked, d.n_seeds = asked, len(seeds)
    for k in range(3):
        t = (2 + k) * TICK
        lst, _ = d.sources(t, 24)
        d.advance(d.tick(t, t + TICK, lst, t + 100, AIR))
    d.sources(40 * TICK, n)                             # (everybody who heard a copy is suppressed in one walk)
    return d


BATCH_FLOOD = dict(imin_us=8 * TICK, doublings=0, max_intervals=4, redundancy=0, seed=2)


def batch_lists(n, ticks=8):
    """tick b holds the nodes j with j % ticks == b; node 9 twice in tick 2, and tick 3 names node 2 again, which sent in tick 2 and
    is not due yet"""
    lists = [[j for j in range(n) if j % ticks == b] for b in range(ticks)]
    lists[2] = lists[2] + [9, 9]
    lists[3] = lists[3] + [2]
    return lists


def scene_batch(make, as_batch):
    """8 self-contained ticks with explicit lists on the lattice, the even nodes seeded: as one batch and an advance per slot, or as
    8 lone ticks with an advance each: the same state"""
    nd = lattice_nodes()
    d = make(nd, "logdist", LATTICE, **BATCH_FLOOD)
    d.seed(list(range(0, nd.n, 2)), 0)
    lists = batch_lists(nd.n)
    tb = [8 * TICK + TICK * b for b in range(len(lists))]
    if as_batch:
        results = d.batch(tb, [t + TICK for t in tb], lists, [t + 100 for t in tb], AIR)
        for b, res in enumerate(results):
            d.advance(res, slot=b)
    else:
        for b, lst in enumerate(lists):
            d.advance(d.tick(tb[b], tb[b] + TICK, lst, tb[b] + 100, AIR))
    return d


def scene_max_hops(make):
    """max_hops 2 on a line: node 3 is never covered"""
    d = make(line_nodes(6), "udgm", UDGM, **dict(LINE, max_hops=2, max_intervals=3))
    d.seed([0], 0)
    run_steps(d, 200, 6)
    return d


def scene_one_interval(make):
    """max_intervals 1 on a clique: every node sends or is suppressed once, then it is done"""
    n = 12
    d = make(clique_nodes(n), "udgm", UDGM, imin_us=1 << 16, doublings=0, max_intervals=1, redundancy=1, seed=5)
    d.seed([0], 0)
    run_steps(d, 200, n, tick=CLIQUE_TICK, air=CLIQUE_AIR)
    return d


def scene_capacity(make):
    """a clique whose second tick has more links than the context's capacity: the slot is lost, nothing changes"""
    n = 12
    d = make(clique_nodes(n), "udgm", UDGM, imin_us=1 << 16, doublings=0, max_intervals=3, redundancy=0, seed=5)
    d.seed([0], 0)
    t = run_steps(d, 1, n, tick=CLIQUE_TICK, air=CLIQUE_AIR)
    d.set_capacity(4)
    before = (d.ref.table(), d.ref.totals())
    run_steps(d, 1, n, t0=t, tick=CLIQUE_TICK, air=CLIQUE_AIR)
    after = d.ref.totals()
    d.unchanged = d.ref.table() == before[0] and {k: v for k, v in after.items() if k != "skipped_slots"} == \
        {k: v for k, v in before[1].items() if k != "skipped_slots"}
    return d
