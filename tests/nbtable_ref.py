"""Reference of the neighbour tables: the rule -- bid, settle, count, expire -- in plain Python integers
over numpy tables, written from the spec alone, the watched links' own pass (E14) over the same results, and the scenes the CPU and
GPU tiers play.  No engine code is involved.  A scene is a function of a DRIVER: the driver owns the reference state, evaluates
ticks (the CPU tier: by the oracle; the GPU tier: by the engine, whose copied-out result then moves the reference) and may compare
after every step.  tests/test_nbtable_ref.py holds the scenes' conditions for the reference alone, so that no GPU test passes
vacuously."""
import numpy as np

from oracle import oracle as O

import cca_ref
import errmodel_ref as EM
import linkstats_ref as LS
import listen_ref as LR
import neighbors_ref as N

DELIVERED = 2          # rm_verdict
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = LS.I64_MIN, LS.I64_MAX
NODE_FIELDS = ("admitted", "evicted_stale", "evicted_poor", "refused", "expired")
TOTALS = ("updates", "skipped_slots") + NODE_FIELDS
DEFAULTS = dict(admit_rssi_dbm=-95.0, timeout_us=60_000_000, min_heard=4, evict_cost=1024, require_delivered=1, reserved=0)


def valid(p):
    a = p["admit_rssi_dbm"]
    return (a == a and abs(a) != float("inf") and 0 <= p["timeout_us"] <= 1 << 62 and 0 <= p["min_heard"] <= 1 << 31
            and (p["evict_cost"] == 0 or 128 <= p["evict_cost"] <= (1 << 32) - 1) and p["require_delivered"] in (0, 1)
            and p.get("reserved", 0) == 0)


def c_in(heard, delivered):
    """E21's entry cost, in uint64"""
    return max(128, ((128 * heard + (delivered >> 1)) & M64) // delivered)


def key(rssi, s):
    """a bid's key: the greatest wins"""
    qc = min(max(int(LS.q8(rssi)), -(1 << 30)), 1 << 30)
    return (qc, -s)


class Result:
    """one slot's result as the update reads it: the packets' src and start_us, pkt_offset, and dst / verdict / rssi (/ sinr, None
    on a medium without the column) per link"""

    def __init__(self, src, start, pkt_offset, dst, verdict, rssi, sinr=None, lost=False):
        self.src = [int(v) for v in src]
        n = len(self.src)
        self.start = [int(start)] * n if np.isscalar(start) else [int(v) for v in start]
        self.pkt_offset = [int(v) for v in pkt_offset]
        self.dst = [int(v) for v in dst]
        self.verdict = [int(v) for v in verdict]
        self.rssi = np.array(rssi, dtype=np.float64)
        self.sinr = None if sinr is None else np.array(sinr, dtype=np.float64)
        self.lost = bool(lost)
        assert len(self.pkt_offset) == n + 1

    def links(self):
        """(p, i, s, d) of every link"""
        for p, s in enumerate(self.src):
            for i in range(self.pkt_offset[p], self.pkt_offset[p + 1]):
                yield p, i, s, self.dst[i]


class State:
    def __init__(self, n, K, **params):
        self.p = dict(DEFAULTS, **params)
        assert valid(self.p)
        self.n, self.K = n, K
        self.tab = LS.Table(n, K)       # (E14's two tables; .peer and .t are written here as well)
        self.clear()
        self.log = {k: 0 for k in ("ties", "empty", "stale", "stale_choice", "poor", "poor_zero_first", "refused", "refused_pinned", "dup_counted",
                                   "undelivered_admitted", "undelivered_bidders", "nan", "low", "bids", "counted_links")}

    def clear(self):
        self.cnt = {f: [0] * self.n for f in NODE_FIELDS}
        self.t = {"updates": 0, "skipped_slots": 0}

    # ---- the rules' words
    def inside(self, j):
        return 0 <= j < self.n

    def empty(self, d, k):
        v = int(self.tab.peer[d, k])
        return not self.inside(v) or v == d

    def pinned(self, d, k, pin):
        return pin is not None and self.inside(int(pin[d])) and int(self.tab.peer[d, k]) == int(pin[d])

    def stale(self, d, k, t):
        to, last = self.p["timeout_us"], int(self.tab.t["last_start_us"][d, k])
        if to <= 0:
            return False
        return last == I64_MIN or (t >= to and last < t - to)

    def poor(self, d, k):
        """-> None, or the order key of (c): delivered == 0 first, then the greatest c_in (then the least k)"""
        H, D = int(self.tab.t["heard"][d, k]), int(self.tab.t["delivered"][d, k])
        if self.p["evict_cost"] <= 0 or H < max(self.p["min_heard"], 1):
            return None
        if D == 0:
            return (1, 0)
        c = c_in(H, D)
        return (0, c) if c > self.p["evict_cost"] else None

    def _clear_entry(self, d, k):
        self.tab.t[d, k] = LS.CLEARED

    def _add(self, d, k, res, p, i):
        e = self.tab.t
        e["heard"][d, k] += np.uint64(1)
        if res.verdict[i] == DELIVERED:
            e["delivered"][d, k] += np.uint64(1)
        e["rssi_q8_sum"][d, k] += LS.q8(res.rssi[i])
        if res.sinr is not None:
            e["sinr_q8_sum"][d, k] += LS.q8(res.sinr[i])
        e["first_start_us"][d, k] = min(int(e["first_start_us"][d, k]), res.start[p])
        e["last_start_us"][d, k] = max(int(e["last_start_us"][d, k]), res.start[p])

    # ---- E14's own pass over a finished slot (what every evaluating call does with the feature on)
    def count(self, res):
        if len(res.src) == 0:
            return
        if res.lost:
            self.tab.skip()
            return
        self.tab.counted += 1
        for p, i, s, d in res.links():
            if self.inside(s) and self.inside(d):
                hit = np.flatnonzero(self.tab.peer[d] == s)
                if len(hit):
                    self._add(d, int(hit[-1]), res, p, i)

    # ---- the calls
    def update(self, res, time_us, pin=None):
        if res.lost:
            self.t["skipped_slots"] += 1
            return
        self.t["updates"] += 1
        P, log = self.p, self.log
        bids, bidders = {}, {}
        for p, i, s, d in res.links():
            if not (self.inside(s) and self.inside(d)) or s == d or (self.tab.peer[d] == s).any():
                continue
            r = float(res.rssi[i])
            if r != r:
                log["nan"] += 1
            elif r < P["admit_rssi_dbm"]:
                log["low"] += 1
            if not r >= P["admit_rssi_dbm"]:
                continue
            if res.verdict[i] != DELIVERED:
                log["undelivered_bidders"] += 1
                if P["require_delivered"]:
                    continue
            log["bids"] += 1
            k = key(r, s)
            bidders.setdefault(d, []).append((k, res.verdict[i]))
            if d not in bids or k > bids[d]:
                bids[d] = k
        admitted = {}
        for d in sorted(bids):
            qc, s = bids[d][0], -bids[d][1]
            if len({k[1] for k, _ in bidders[d] if k[0] == qc}) > 1:
                log["ties"] += 1
            slot, kind = None, None
            empties = [k for k in range(self.K) if self.empty(d, k)]
            if empties:
                slot, kind = empties[0], "empty"
            if slot is None:
                stale = [(int(self.tab.t["last_start_us"][d, k]), k) for k in range(self.K) if not self.pinned(d, k, pin) and self.stale(d, k, time_us)]
                if stale:
                    slot, kind = min(stale)[1], "stale"
                    log["stale_choice"] += len(stale) > 1
            if slot is None:
                poor = [(self.poor(d, k), k) for k in range(self.K) if not self.pinned(d, k, pin) and self.poor(d, k) is not None]
                if poor:
                    best = max(v for v, _ in poor)
                    slot, kind = min(k for v, k in poor if v == best), "poor"
                    log["poor_zero_first"] += best[0] == 1 and any(v[0] == 0 for v, _ in poor)
            if slot is None:
                self.cnt["refused"][d] += 1
                log["refused"] += 1
                log["refused_pinned"] += any(self.pinned(d, k, pin) for k in range(self.K))
                continue
            log[kind] += 1
            if kind != "empty":
                self.cnt["evicted_" + kind][d] += 1
            self.tab.peer[d, slot] = s
            self._clear_entry(d, slot)
            self.cnt["admitted"][d] += 1
            admitted[d] = (s, slot)
            if all(v != DELIVERED for k, v in bidders[d] if k == bids[d]):
                log["undelivered_admitted"] += 1
        per = {}
        for p, i, s, d in res.links():
            if d in admitted and admitted[d][0] == s and self.inside(s):
                self._add(d, admitted[d][1], res, p, i)
                per[d] = per.get(d, 0) + 1
                log["counted_links"] += 1
        log["dup_counted"] += sum(1 for v in per.values() if v > 1)

    def expire(self, time_us, pin=None):
        for d in range(self.n):
            for k in range(self.K):
                if self.empty(d, k) or self.pinned(d, k, pin) or not self.stale(d, k, time_us):
                    continue
                self.tab.peer[d, k] = -1
                self._clear_entry(d, k)
                self.cnt["expired"][d] += 1

    def reset(self):
        self.clear()

    # ---- what the reads return
    def totals(self):
        t = {f: sum(self.cnt[f]) for f in NODE_FIELDS}
        t.update(self.t, reserved=0)
        return t

    def check(self):
        """the identities and the row invariant"""
        for d in range(self.n):
            assert self.cnt["admitted"][d] >= self.cnt["evicted_stale"][d] + self.cnt["evicted_poor"][d], d
            held = [int(v) for v in self.tab.peer[d] if self.inside(int(v)) and int(v) != d]
            assert len(set(held)) == len(held), (d, held)


# ---- drivers ---------------------------------------------------------------------------------------------------------------------

KIND = {"null": 0, "udgm": 1, "logdist": 4}
TICK, AIR = 5000, 4256
UDGM = {"udgm_transmission_range": 50.0, "udgm_interference_range": 100.0}


def has_sinr(kind, params):
    return kind == "logdist" and bool(int(params.get("ld_flags", 0)) & 1)


class Driver:
    """the CPU tier's driver: the reference state over ticks the oracle evaluates.  The GPU tier subclasses it
    (tests/test_gpu_nbtable.py): every call also goes to the engine, ticks are the engine's, and the two states are compared after
    every call.  listen: E13's schedule table or None; errmodel: E10's seed or None"""

    def __init__(self, nd, kind, params, K, listen=None, errmodel=None, **nbt):
        self.nd, self.kind, self.params, self.listen, self.errmodel = nd, kind, dict(params), listen, errmodel
        self.K = K
        self.ref = State(nd.n, K, **nbt)
        self.sinr = has_sinr(kind, params)
        self.chain = None
        self.capacity = None
        self.steps = 0

    # -- evaluation by the oracle
    def _chain(self):
        if self.chain is None:
            self.chain = cca_ref.Chain(O, self.nd, O.model(KIND[self.kind], **self.params))
        return self.chain

    def result(self, src, start, pkt_offset, dst, verdict, rssi, sinr, lost=False):
        """a tick over a source list: the record of an entry outside the table has src -1"""
        s = np.asarray(src, dtype=np.int64)
        ok = (s >= 0) & (s < self.nd.n)
        return Result(np.where(ok, s, -1), start, pkt_offset, dst, verdict, rssi, sinr if self.sinr else None, lost)

    def _expected(self, src, e, start):
        verdict = e.verdict
        if e.raw is not None:
            if self.errmodel is not None:
                verdict = EM.apply_full(e.new, e.raw, self.errmodel)[0]
            if self.listen is not None:
                verdict, _ = LR.apply(e.new, e.raw, self.listen, verdict)
        lost = self.capacity is not None and e.count > self.capacity
        if lost:
            return self.result(src, start, [0] * (len(src) + 1), [], [], [], [], True)
        return self.result(src, start, e.pkt_offset, e.dst, verdict, e.rssi, e.sinr)

    def set_capacity(self, cap):
        """the context's link capacity: a tick with more heard links is lost"""
        self.capacity = cap

    def tick(self, t_begin, t_end, src, start, air):
        """a plain lone tick over the source list (padding: outside the table), E14's pass behind it -> Result"""
        res = self._expected(src, self._chain().plain_tick(t_begin, src, start, air), start)
        self.ref.count(res)
        return res

    def batch(self, t_begin, t_end, lists, starts, air):
        """a batch of self-contained ticks: E14 counts ALL of them before the first update can run"""
        return [self.tick(t_begin[b], t_end[b], lists[b], starts[b], air) for b in range(len(lists))]

    # -- the calls
    def update(self, res, time_us, pin=None, slot=0):
        self.ref.update(res, time_us, pin)
        self.steps += 1
        self.after("update")

    def expire(self, time_us, pin=None):
        self.ref.expire(time_us, pin)
        self.after("expire")

    def watch(self, nodes, rows):
        self.ref.tab.watch(nodes, rows)
        self.after("watch")

    def stats_reset(self):
        """rm_linkstats_reset: every entry cleared, so every watched entry is stale"""
        self.ref.tab.reset()
        self.after("linkstats_reset")

    def reset(self):
        self.ref.reset()
        self.after("reset")

    def after(self, what):
        self.ref.check()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

def line_nodes(n, pitch=40.0):
    nd = O.NodeTable(n)
    nd.x = pitch * np.arange(n)
    nd.txpower = np.zeros(n)
    return nd


def clique_nodes(n, radius=15.0):
    """n nodes on a disc: everybody hears everybody (UDGM 50 / 100, and the log-distance defaults at txpower 0)"""
    nd = O.NodeTable(n)
    rng = np.random.default_rng(n)
    r, a = radius * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    nd.x, nd.y = r * np.cos(a), r * np.sin(a)
    nd.txpower = np.zeros(n)
    return nd


def lattice_nodes(side=9, pitch=50.0):
    """side x side nodes `pitch` apart, txpower 0: under the log-distance defaults (reach 68 m) the four neighbours are heard"""
    nd = O.NodeTable(side * side)
    k = np.arange(side * side)
    nd.x, nd.y = pitch * (k % side), pitch * (k // side)
    nd.txpower = np.zeros(side * side)
    return nd


def rounds(d, lists, t0=0, pin=None, update=True):
    """one lone tick per list, an update behind each -> the time after the last"""
    t = t0
    for lst in lists:
        res = d.tick(t, t + TICK, lst, t + 100, AIR)
        if update:
            d.update(res, t + TICK, pin)
        t += TICK
    return t


def stride_lists(n, ticks, stride):
    """tick b: the nodes j with j % stride == b % stride"""
    return [[j for j in range(n) if j % stride == b % stride] for b in range(ticks)]


FILL = dict(timeout_us=0, evict_cost=0)


def scene_fill(make, shape, n, K, ticks=8):
    """tables from empty on a line (log-distance, 20 m apart: three neighbours on either side, pairwise at one rssi) or a clique
    (UDGM: constant rssi, every bid a tie), filled over several ticks: one admission per node and tick"""
    if shape == "line":
        d = make(line_nodes(n, 20.0), "logdist", N.PLAIN, K, **FILL)
        rounds(d, stride_lists(n, ticks, 4))
    else:
        d = make(clique_nodes(n), "udgm", UDGM, K, **FILL)
        rounds(d, stride_lists(n, ticks, 4))
    return d


def scene_long(make):
    """a 192-node clique, 96 transmitters in one tick: 96 * 191 = 18 336 links; then a second tick of the other half"""
    n = 192
    d = make(clique_nodes(n), "udgm", UDGM, 4, **FILL)
    rounds(d, [list(range(0, n, 2)), list(range(1, n, 2))])
    return d


def field_nodes(n, seed=3, k=12.0):
    nd, _ = cca_ref.uniform_nodes(O, n, seed, k=k)
    nd.txpower = np.zeros(n)
    return nd


def scene_big(make, n):
    """a random field: every fourth node sends, three ticks; then an expire that keeps only what the last tick heard"""
    d = make(field_nodes(n), "logdist", N.PLAIN, 4, timeout_us=2 * TICK, evict_cost=0)
    t = rounds(d, stride_lists(n, 3, 4))
    d.expire(t + 200)
    return d


LATTICE = dict(N.PLAIN, **dict(N.SINR, ld_capture_db=-1.0))


def lattice_listen(n):
    """E13 for every fifth node: awake 3 ms of every 7 ms"""
    return [(7000, 3000, (131 * j) % 7000) if j % 5 == 2 else (0, 0, 0) for j in range(n)]


def scene_media(make, require_delivered, side=33, ticks=6):
    """side x side, 30 m apart (20 neighbours in reach, the outer 8 below admit_rssi_dbm), on the SINR medium with duty-cycled
    receivers and the frame error model: collided and missed copies bid only with require_delivered = 0"""
    nd = lattice_nodes(side, 30.0)
    d = make(nd, "logdist", LATTICE, 4, listen=lattice_listen(nd.n), errmodel=77, timeout_us=0, evict_cost=0, require_delivered=require_delivered,
             admit_rssi_dbm=-92.0)
    rounds(d, stride_lists(nd.n, ticks, 4))       # (33 = 1 mod 4: the neighbours to the right and below send together, equally strong)
    return d


def scene_tie(make):
    """UDGM, constant rssi: nodes 1 and 2 send in one tick, node 0 hears both at one strength and admits the lower index"""
    d = make(line_nodes(3, 10.0), "udgm", UDGM, 1, **FILL)
    rounds(d, [[2, 1]])
    return d


EDGE = dict(timeout_us=4 * TICK, min_heard=2, evict_cost=200, require_delivered=0)


def scene_evict(make):
    """a 6-node clique on the SINR medium with K = 2.  Node 0 learns 1 and 2; 1 goes quiet and 2 follows later: two stale slots,
    the older one goes to 3.  Then rows are set by hand to show the poor line: a slot that never delivered beats one with a high
    cost, and with every slot healthy or pinned the bid is refused"""
    n = 6
    d = make(clique_nodes(n, 5.0), "logdist", dict(N.PLAIN, **N.SINR), 2, **EDGE)
    t = rounds(d, [[1], [2], [2]])                            # node 0: slots {1, 2}; 2 heard later than 1
    t = rounds(d, [[5]] * 8, t0=t + 8 * TICK, update=False)   # (time passes; 5 is heard by nobody's table: no update)
    rounds(d, [[3]], t0=t)                                    # every row is full of stale peers: the older slot goes
    return d


def scene_poor(make):
    """K = 2 on a line on the SINR medium, senders paired so that the weaker copy collides: node 0's row holds a peer that never
    delivered and a merely costly one, and a newcomer takes the former; a pinned poor slot is passed over and a row of pinned and
    fresh slots refuses"""
    n = 8
    nd = O.NodeTable(n)
    nd.x = np.array([-2.0, 4.0, 10.0, 0.0, -3.0, -4.0, 14.0, 15.0])     # at node 0: 3 is stronger than 1, 1 stronger than 2
    nd.txpower = np.zeros(n)
    d = make(nd, "logdist", dict(N.PLAIN, **dict(N.SINR, ld_capture_db=3.0)), 2, timeout_us=0, min_heard=2, evict_cost=200, require_delivered=0)
    t = rounds(d, [[1, 2]] * 3)                           # node 0 learns 1, then 2 from a collided copy: 2's entry stays at delivered == 0
    t = rounds(d, [[1, 3]] * 4, t0=t, update=False)       # 3 drowns 1 at node 0: 1's entry turns costly, with delivered > 0
    pin = np.full(n, -1, dtype=np.int32)
    t = rounds(d, [[4]], t0=t, pin=pin)                   # 4 takes the delivered == 0 slot (2's), not the costly one
    pin[:] = 1
    pin[4] = -7                                           # (outside the table: pins nothing)
    t = rounds(d, [[5]] * 3, t0=t, pin=pin)               # at node 0, 1 is pinned and 4 is fresh: 5 is refused
    return d


def scene_pins(make):
    """K = 1: the only slot pinned refuses every bid; timeout_us = 0 and evict_cost = 0 disable their lines; t < timeout_us"""
    n = 5
    d = make(clique_nodes(n, 5.0), "udgm", UDGM, 1, timeout_us=1 << 40, evict_cost=0)
    t = rounds(d, [[0], [1]])                                   # everybody holds 0 (node 0 holds 1)
    d.watch([4], [[3]])                                         # a watched entry that never heard anything: stale at any t < timeout_us
    pin = np.array([1, 0, 0, 0, -7], dtype=np.int32)
    t = rounds(d, [[2]], t0=t, pin=pin)                         # pinned rows refuse; node 4's stale slot goes to 2
    t = rounds(d, [[3]], t0=t, pin=None)                        # t < timeout_us and last_start_us set: nobody is stale, all refuse
    d.expire(t, pin)
    return d


def scene_disabled(make):
    """timeout_us = 0 and evict_cost = 0: full rows refuse for ever, expire removes nothing"""
    n = 5
    d = make(clique_nodes(n, 5.0), "udgm", UDGM, 1, timeout_us=0, evict_cost=0)
    t = rounds(d, [[0], [1], [2], [3]])
    d.expire(1 << 50)
    return d


def scene_capacity(make):
    """a clique whose second tick has more links than the context's capacity: skipped_slots == 1 and nothing else changes"""
    n = 12
    d = make(clique_nodes(n), "udgm", UDGM, 2, **FILL)
    t = rounds(d, [[0]])
    d.set_capacity(4)
    before = (d.ref.tab.peer.copy(), d.ref.tab.t.copy(), {f: list(v) for f, v in d.ref.cnt.items()}, dict(d.ref.totals()))
    rounds(d, [[1, 2]], t0=t)
    after = d.ref.totals()
    d.unchanged = ((d.ref.tab.peer == before[0]).all() and d.ref.tab.t.tobytes() == before[1].tobytes() and d.ref.cnt == before[2]
                   and {k: v for k, v in after.items() if k != "skipped_slots"} == {k: v for k, v in before[3].items() if k != "skipped_slots"})
    return d


def batch_lists(n, ticks=8):
    """tick b: the nodes j with j % 4 == b % 4 -- every sender returns four ticks later"""
    return stride_lists(n, ticks, 4)


def scene_batch(make, as_batch):
    """8 self-contained ticks on the 9 x 9 lattice from an empty table: as one batch with an update per slot in ascending order --
    E14 has counted all eight ticks before the first update, so a peer admitted from slot b misses its frames of the later slots --
    or as 8 lone ticks with an update each, where they are counted"""
    nd = lattice_nodes()
    d = make(nd, "logdist", LATTICE, 4, **FILL)
    lists = batch_lists(nd.n)
    tb = [TICK * b for b in range(len(lists))]
    if as_batch:
        results = d.batch(tb, [t + TICK for t in tb], lists, [t + 100 for t in tb], AIR)
        for b, res in enumerate(results):
            d.update(res, tb[b] + TICK, slot=b)
    else:
        rounds(d, lists)
    return d


def scene_dup(make):
    """a source twice in one list: two frames, two links to every receiver, both counted into the fresh entry"""
    d = make(clique_nodes(4, 5.0), "udgm", UDGM, 2, **FILL)
    rounds(d, [[1, 1]])
    return d


def scene_weak(make):
    """a line 30 m apart under the log-distance defaults with admit_rssi_dbm = -86: the 60 m links (-93.3 dBm) are heard and never
    bid"""
    d = make(line_nodes(8, 30.0), "logdist", N.PLAIN, 4, admit_rssi_dbm=-86.0, timeout_us=0, evict_cost=0)
    rounds(d, stride_lists(8, 4, 2))
    return d
