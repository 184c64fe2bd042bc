"""Reference of the forwarding queues: a plain-Python state machine written from the rules alone --
lists of packets per node, Python integers --, and the scenes the CPU and GPU tiers play.  No engine code is involved.  A scene is a
function of a DRIVER: the driver owns the reference state, evaluates ticks (the CPU tier: by the oracle; the GPU tier: by the engine,
whose copied-out result then advances the reference) and may compare after every step.  tests/test_fwd_ref.py holds the scenes'
conditions for the reference alone, so that no GPU test passes vacuously."""
import numpy as np

from oracle import oracle as O

import cca_ref
import hops_ref as H
import neighbors_ref as N
import traffic_ref as T

NO_ROUTE, SINK = -1, -2
DELIVERED = 2          # rm_verdict
M64 = (1 << 64) - 1
NODE_FIELDS = ("generated", "arrived", "lost", "latency_us_sum", "latency_us_max", "hops_sum", "attempts", "acked", "failed", "deferred",
               "rejected", "dropped", "ready_us", "next", "queue_len", "queue_max", "tries")
TOTALS = ("generated", "arrived", "dropped_retries", "dropped_no_route", "dropped_full", "dropped_ttl", "in_flight", "stray", "skipped_slots",
          "latency_us_sum", "hops_sum")
DEFAULTS = dict(queue_slots=8, max_retries=3, min_be=3, max_be=5, max_hops=64, backoff_unit_us=320, seed=0, reserved=0)


def valid(p):
    return (p["queue_slots"] in (1, 2, 4, 8, 16) and 0 <= p["max_retries"] <= 15 and 0 <= p["min_be"] <= p["max_be"] <= 8
            and 1 <= p["max_hops"] <= 255 and 0 <= p["backoff_unit_us"] <= 1 << 32 and p.get("reserved", 0) == 0)


def backoff_factor(p, node, start_us, tries):
    be = min(p["min_be"] + tries - 1, p["max_be"])
    if be == 0:
        return 0
    h1 = T.mix64(T.mix64(T.mix64((p["seed"] + T.GOLDEN) & M64) ^ (node & 0xFFFFFFFF)) ^ (start_us & M64))
    h2 = T.mix64(h1 ^ tries)
    return h2 >> (64 - be)


class Result:
    """one slot's result as the advance reads it: the tx records' src / start / air per packet number, pkt_offset, dst, verdict"""

    def __init__(self, src, start, air, pkt_offset, dst, verdict, lost=False):
        self.src = [int(v) for v in src]
        n = len(self.src)
        self.start = [int(start)] * n if np.isscalar(start) else [int(v) for v in start]
        self.air = [int(air)] * n if np.isscalar(air) else [int(v) for v in air]
        self.pkt_offset = [int(v) for v in pkt_offset]
        self.dst = [int(v) for v in dst]
        self.verdict = [int(v) for v in verdict]
        self.lost = bool(lost)
        assert len(self.pkt_offset) == n + 1

    def delivered(self, p, w, n_nodes):
        """E12: the status of (p, w) is DELIVERED"""
        if w < 0 or not 0 <= self.src[p] < n_nodes:
            return False
        for i in range(self.pkt_offset[p], self.pkt_offset[p + 1]):
            if self.dst[i] == w:
                return self.verdict[i] == DELIVERED
        return False


def records_result(n_nodes, src, start, air, pkt_offset, dst, verdict):
    """a tick over a source list: the record of an entry outside the table -- padding, or a candidate the gate deferred -- has
    src -1 and air_us 0 (what the device ticks write for such a slot), every other one the tick's air time"""
    s = np.asarray(src, dtype=np.int64)
    ok = (s >= 0) & (s < n_nodes)
    return Result(np.where(ok, s, -1), [int(start)] * len(s), np.where(ok, int(air), 0), pkt_offset, dst, verdict)


class State:
    """packets are tuples (enq_us, birth_us, origin, hops): the tuple order is the queue order"""

    def __init__(self, n, **params):
        self.p = dict(DEFAULTS, **params)
        assert valid(self.p)
        self.n = n
        self.next = [NO_ROUTE] * n
        self.clear()

    def clear(self):
        n = self.n
        self.q = [[] for _ in range(n)]
        self.tries = [0] * n
        self.ready = [0] * n
        self.c = {f: [0] * n for f in NODE_FIELDS[:12] + ("queue_max",)}
        self.t = {f: 0 for f in TOTALS if f != "in_flight"}

    # ---- the rules' words
    def head(self, j):
        return min(self.q[j])

    def sendable(self, j, t):
        return bool(self.q[j]) and self.ready[j] <= t and self.head(j)[0] <= t

    def _arrive(self, pkt, t, hops):
        o = pkt[2]
        lat = t - pkt[1]
        self.c["arrived"][o] += 1
        self.c["latency_us_sum"][o] += lat
        self.c["latency_us_max"][o] = max(self.c["latency_us_max"][o], lat)
        self.c["hops_sum"][o] += hops
        self.t["arrived"] += 1
        self.t["latency_us_sum"] += lat
        self.t["hops_sum"] += hops

    def _drop(self, pkt, at, why):
        self.c["lost"][pkt[2]] += 1
        self.c["dropped"][at] += 1
        self.t["dropped_" + why] += 1

    def _push(self, w, pkt, len_base, k):
        self.q[w].append(pkt)
        self.c["queue_max"][w] = max(self.c["queue_max"][w], len_base + k)

    # ---- the calls
    def set_next(self, parent, roots, time_us):
        n = self.n
        assert len(parent) == n
        for j in range(n):
            v = int(parent[j])
            self.next[j] = v if (0 <= v < n and v != j) else NO_ROUTE
        for r in roots:
            if 0 <= int(r) < n:
                self.next[int(r)] = SINK
        for j in range(n):
            if self.next[j] >= 0:
                continue
            for pkt in self.q[j]:
                if self.next[j] == SINK:
                    self._arrive(pkt, time_us, pkt[3])
                else:
                    self._drop(pkt, j, "no_route")
            self.q[j] = []
            self.tries[j] = 0

    def inject(self, src, time_us):
        start_len = [len(q) for q in self.q]
        pushed = {}
        for j in src:
            j = int(j)
            if not 0 <= j < self.n:
                continue
            self.c["generated"][j] += 1
            self.t["generated"] += 1
            pkt = (time_us, time_us, j, 0)
            if self.next[j] == SINK:
                self._arrive(pkt, time_us, 0)
            elif self.next[j] == NO_ROUTE:
                self._drop(pkt, j, "no_route")
            elif len(self.q[j]) >= self.p["queue_slots"]:
                self._drop(pkt, j, "full")
            else:
                pushed[j] = pushed.get(j, 0) + 1
                self._push(j, pkt, start_len[j], pushed[j])

    def sources(self, time_us, cap):
        s = [j for j in range(self.n) if self.sendable(j, time_us)]
        return (s + [-1] * cap)[:cap], len(s)

    def advance(self, res, cand=None):
        """one slot's result; cand: the candidate list handed to the evaluating call, or None"""
        if res.lost:
            self.t["skipped_slots"] += 1
            return
        n_new = len(res.src)
        P = n_new if cand is None else min(len(cand), n_new)
        Q = self.p["queue_slots"]
        len_start = [len(q) for q in self.q]
        seen, part = set(), []      # the participants: (p, j, w, head, case), judged on the state at the start of the call
        for p in range(P):
            j = int(res.src[p] if cand is None else cand[p])
            if not 0 <= j < self.n:
                continue
            if j in seen or not self.sendable(j, res.start[p]):
                seen.add(j)
                self.t["stray"] += 1
                continue
            seen.add(j)
            w = self.next[j]
            assert w >= 0
            if res.src[p] != j:
                case = "deferred"
            elif not res.delivered(p, w, self.n):
                case = "failed"
            else:
                case = "sink" if self.next[w] == SINK else "relay"
            part.append((p, j, w, self.head(j), case))
        A = {}
        for _, _, w, _, case in part:
            if case == "relay":
                A[w] = A.get(w, 0) + 1
        pushed = {}
        for p, j, w, head, case in part:
            t_end = res.start[p] + res.air[p]
            self.c["attempts"][j] += 1
            rejected = case == "relay" and len_start[w] + A[w] > Q
            if case in ("sink", "relay") and not rejected:
                self.q[j].remove(head)
                self.tries[j], self.ready[j] = 0, t_end
                self.c["acked"][j] += 1
                enq, birth, origin, hops = head
                if case == "sink":
                    self._arrive(head, t_end, hops + 1)
                elif hops + 1 > self.p["max_hops"]:
                    self._drop(head, w, "ttl")
                else:
                    pushed[w] = pushed.get(w, 0) + 1
                    self._push(w, (t_end, birth, origin, hops + 1), len_start[w], pushed[w])
                continue
            self.c["deferred" if case == "deferred" else "failed"][j] += 1
            if rejected:
                self.c["rejected"][w] += 1
            self.tries[j] += 1
            if self.tries[j] > self.p["max_retries"]:
                self.q[j].remove(head)
                self._drop(head, j, "retries")
                self.tries[j], self.ready[j] = 0, t_end
            else:
                self.ready[j] = t_end + backoff_factor(self.p, j, res.start[p], self.tries[j]) * self.p["backoff_unit_us"]

    # ---- what the reads return
    def totals(self):
        t = dict(self.t)
        t["in_flight"] = sum(len(q) for q in self.q)
        return t

    def table(self):
        out = {f: list(self.c[f]) for f in self.c}
        out["ready_us"], out["next"], out["tries"] = list(self.ready), list(self.next), list(self.tries)
        out["queue_len"] = [len(q) for q in self.q]
        return out

    def queues(self):
        """per node the packets in queue order as (origin, hops, birth_us, enq_us)"""
        return [[(o, h, b, e) for e, b, o, h in sorted(q)] for q in self.q]

    def check(self):
        """the two identities and the invariant"""
        t = self.totals()
        assert t["generated"] == t["arrived"] + t["dropped_retries"] + t["dropped_no_route"] + t["dropped_full"] + t["dropped_ttl"] + t["in_flight"], t
        c = self.c
        for j in range(self.n):
            assert c["attempts"][j] == c["acked"][j] + c["failed"][j] + c["deferred"][j], j
            assert not self.q[j] or self.next[j] >= 0, j
            assert len(self.q[j]) <= self.p["queue_slots"], j
        assert sum(c["generated"]) == t["generated"] and sum(c["arrived"]) == t["arrived"]
        assert sum(c["lost"]) == sum(c["dropped"]) == t["generated"] - t["arrived"] - t["in_flight"]


# ---- drivers ---------------------------------------------------------------------------------------------------------------------

class Driver:
    """the CPU tier's driver: the reference state over ticks the oracle evaluates.  The GPU tier subclasses it (tests/test_gpu_fwd.py):
    every call also goes to the engine, ticks are the engine's, and the two states are compared after every step"""

    def __init__(self, nd, kind, params, **fwd):
        self.nd, self.kind, self.params = nd, kind, dict(params)
        self.ref = State(nd.n, **fwd)
        self.chain = None
        self.log = {"deferred_lists": 0, "truncated": 0, "steps": 0}

    # -- evaluation by the oracle
    def _chain(self):
        if self.chain is None:
            kw = dict(self.params)
            self.chain = cca_ref.Chain(O, self.nd, O.model(KIND[self.kind], **kw))
        return self.chain

    def tick(self, t_begin, t_end, src, start, air):
        """a plain lone tick over the source list (padding: outside the table) -> Result"""
        e = self._chain().plain_tick(t_begin, src, start, air)
        return self._result(src, e, start, air)

    def tick_cca(self, t_begin, t_end, src, start, air, cca_time, threshold):
        """a gated lone tick -> Result (a deferred candidate's record has src -1)"""
        flags, _, e = self._chain().gated_tick(t_begin, src, start, air, cca_time, threshold)
        kept = np.where(flags != 0, -1, np.asarray(src, dtype=np.int32))
        return self._result(kept, e, start, air)

    def _result(self, src, e, start, air):
        s = np.asarray(src, dtype=np.int64)
        return records_result(self.nd.n, s, start, air, e.pkt_offset, e.dst, e.verdict)

    # -- the feature's calls
    def set_next(self, parent, roots, time_us):
        self.ref.set_next(parent, roots, time_us)
        self.after("set_next")

    def inject(self, src, time_us):
        self.ref.inject(src, time_us)
        self.after("inject")

    def set_traffic(self, table, seed):
        """E15's schedules: inject_traffic(lo, hi) injects the row of the window [lo, hi), whole (n = cap = n_nodes), at lo"""
        self.traffic = (table, seed)

    def traffic_row(self, lo, hi):
        rows, _, _, _ = T.generate(self.traffic[0], self.traffic[1], [lo], [hi], self.nd.n)
        return [int(v) for v in rows[0]]

    def inject_traffic(self, lo, hi):
        self.ref.inject(self.traffic_row(lo, hi), lo)
        self.after("inject")

    def sources(self, time_us, cap):
        lst, count = self.ref.sources(time_us, cap)
        if count > cap:
            self.log["truncated"] += 1
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

    def tree(self, roots):
        """the hop query's parents toward `roots` (HEARD_BY) -> parent list (the CPU tier: tests/hops_ref.py)"""
        found = N.links(self.nd, {k: v for k, v in self.params.items()}, H.HEARD_BY)
        return [int(v) for v in H.tree(self.nd.n, found, roots)["parent"]]


KIND = {"null": 0, "udgm": 1, "logdist": 4}
TICK, AIR = 5000, 4256


def run_steps(d, n_steps, cap, t0=0, tick=TICK, air=AIR, start_at=100, traffic=False, until_empty=False):
    """step k at t = t0 + k * tick: (traffic(k) injected), the sendable nodes' list, a lone tick of it, the advance"""
    k = 0
    while k < n_steps:
        t = t0 + k * tick
        if traffic:
            d.inject_traffic(t, t + tick)
        lst, count = d.sources(t + start_at, cap)
        d.advance(d.tick(t, t + tick, lst, t + start_at, air))
        k += 1
        if until_empty and d.ref.totals()["in_flight"] == 0:
            break
    return k


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

def line_nodes(n):
    """n nodes in a row 40 m apart: under UDGM 50 / 100 node i's frame reaches i - 1 and i + 1 and disturbs i - 2 and i + 2"""
    nd = O.NodeTable(n)
    nd.x = 40.0 * np.arange(n)
    return nd


LINE_FWD = dict(queue_slots=16, max_retries=15, min_be=2, max_be=5, max_hops=255, backoff_unit_us=TICK, seed=7)


def scene_line(make, n):
    """the sink at one end, one packet per node: every packet arrives with hops = its distance"""
    d = make(line_nodes(n), "udgm", {"udgm_transmission_range": 50.0, "udgm_interference_range": 100.0}, **LINE_FWD)
    d.set_next(list(range(-1, n - 1)), [0], 0)
    d.inject(list(range(n)), 0)
    run_steps(d, 6000, n, until_empty=True)
    return d


def hub_nodes(leaves):
    """leaves 0 .. L - 1, the hub L, one more node L + 1 behind the hub"""
    nd = O.NodeTable(leaves + 2)
    rng = np.random.default_rng(leaves)
    nd.x, nd.y = rng.uniform(0, 100.0, leaves + 2), rng.uniform(0, 100.0, leaves + 2)
    return nd


def scene_hub_sink(make, leaves):
    """every leaf sends in one tick to the hub, a sink: one counter address hit from several waves and blocks"""
    d = make(hub_nodes(leaves), "null", {}, queue_slots=16)
    d.set_next([leaves] * leaves + [-1, -1], [leaves], 0)
    d.inject(list(range(leaves)), 10)
    run_steps(d, 1, leaves + 3)
    return d


def scene_hub_relay(make, arrivals, preload):
    """the hub a relay under Q = 16 with `preload` packets of its own: `arrivals` leaves send in one tick"""
    leaves = 20
    d = make(hub_nodes(leaves), "null", {}, queue_slots=16, max_retries=3)
    d.set_next([leaves] * leaves + [leaves + 1, -1], [leaves + 1], 0)
    d.inject([leaves] * preload + list(range(arrivals)), 10)
    run_steps(d, 1, leaves + 2)
    return d


def lattice_nodes(side=9, pitch=50.0):
    """side x side nodes `pitch` apart, txpower 0: under the log-distance defaults (reach 68 m) the four neighbours are heard"""
    nd = O.NodeTable(side * side)
    k = np.arange(side * side)
    nd.x, nd.y = pitch * (k % side), pitch * (k // side)
    nd.txpower = np.zeros(side * side)
    return nd


LATTICE = dict(N.PLAIN, **N.SINR)
LATTICE_TRAFFIC = (400000, 1000)   # period_us, jitter_us of every node but the sink


def lattice_table(n, sink):
    """E15's table: node j has period 400 ms, phase (977 j) mod period, a little jitter; the sink has no schedule"""
    period, jitter = LATTICE_TRAFFIC
    return [(0, 0, 0) if j == sink else (period, (977 * j) % period, jitter) for j in range(n)]


def scene_lattice(make, max_retries, min_be, max_be, steps=200, cca=None, cand=True):
    """9 x 9, log-distance with SINR, next from the hop query toward the corner, E15's traffic, plain lone ticks: collisions give
    retries, backoffs and drops.  cca = (sample_at, threshold): the ticks are gated, frames outlive their tick (tick 1000 us) and
    the candidate list goes to the advance (cand) or not"""
    nd = lattice_nodes()
    d = make(nd, "logdist", LATTICE, queue_slots=4, max_retries=max_retries, min_be=min_be, max_be=max_be, max_hops=64,
             backoff_unit_us=1000, seed=11)
    d.set_next(d.tree([0]), [0], 0)
    d.set_traffic(lattice_table(nd.n, 0), 5)
    if cca is None:
        run_steps(d, steps, nd.n, traffic=True)
        return d
    tick = 1000
    for k in range(steps):
        t = k * tick
        d.inject_traffic(t, t + tick)
        lst, count = d.sources(t + 200, nd.n)
        res = d.tick_cca(t, t + tick, lst, t + 200, AIR, t + 128, cca[1])
        if any(s != c for s, c in zip(res.src, lst) if 0 <= c < nd.n):
            d.log["deferred_lists"] += 1
        d.advance(res, lst if cand else None)
    return d


def field_nodes(n, seed=3, k=12.0):
    nd, _ = cca_ref.uniform_nodes(O, n, seed, k=k)
    nd.txpower = np.zeros(n)
    return nd


def scene_big(make, n):
    """a random field; the queues are loaded by injection alone, and the source list is asked with 0, 1, cap - 1, cap and cap + 1
    sendable nodes that sit on both sides of every 256 and 1024 boundary; then one tick of a short list and its advance"""
    d = make(field_nodes(n), "logdist", N.PLAIN, queue_slots=2, max_retries=1)
    d.set_next([(j + 1) % n for j in range(n)], [n - 1], 0)
    asked = []
    lst, c = d.sources(5, 7)
    asked.append((c, 7))
    edge = sorted({j for b in range(256, n, 256) for j in (b - 1, b)} | {0, n - 2})
    d.inject(edge[:1], 10)
    asked.append((d.sources(10, 7)[1], 7))
    d.inject(edge[1:], 20)
    d.inject(edge[::2], 30)      # (a second packet at every other one: full queues next to short ones)
    m = d.ref.sources(30, 1)[1]   # (the sink among them took its packet at once)
    for cap in (m + 1, m, m - 1, 1):
        lst, c = d.sources(30, cap)
        asked.append((c, cap))
    lst, c = d.sources(25, m)    # (the later packets are not at the head: every loaded node is sendable by its first)
    asked.append((c, m))
    lst, c = d.sources(15, m)    # (between the two injections: the first node alone)
    asked.append((c, m))
    d.loaded = d.ref.sources(30, n)[0]
    t = TICK
    lst, _ = d.sources(t, 24)
    d.advance(d.tick(t, t + TICK, lst, t + 100, AIR))
    d.asked = asked
    return d


def scene_reroute(make):
    """a line of 8 toward node 0; in mid-run node 3, loaded, becomes a sink (its queue arrives), node 5 loses its route (its queue is
    dropped), and 6 <-> 7 become a 2-cycle that max_hops = 4 ends"""
    n = 8
    d = make(line_nodes(n), "udgm", {"udgm_transmission_range": 50.0, "udgm_interference_range": 100.0}, queue_slots=4, max_retries=15,
             min_be=1, max_be=3, max_hops=4, backoff_unit_us=TICK, seed=3)
    d.set_next(list(range(-1, n - 1)), [0], 0)
    d.inject([3, 3, 5, 5, 5, 6, 7], 0)
    parent = list(range(-1, n - 1))
    parent[5], parent[6], parent[7] = 5, 7, 6     # (itself: no route)
    d.set_next(parent, [0, 3], 777)
    run_steps(d, 400, n, t0=TICK, until_empty=True)
    return d


def batch_lists(n, ticks=8):
    """node-disjoint lists: tick b holds the nodes j with j % ticks == b (but the sink), node 9 one tick later, so that node 1 is
    alone next to the sink in tick 1; nodes 2 and 10 collide at node 1 in tick 2, and tick 5 names node 2 again, in backoff"""
    lists = [[j for j in range(1, n) if j % ticks == b and j != 9] for b in range(ticks)]
    lists[2] = lists[2] + [9]
    lists[5] = lists[5] + [2]
    return lists


def scene_batch(make, as_batch):
    """8 self-contained ticks with node-disjoint lists on the lattice, as one batch and an advance per slot, or as 8 lone ticks with
    an advance each: the same state"""
    nd = lattice_nodes()
    d = make(nd, "logdist", LATTICE, queue_slots=4, max_retries=2, min_be=8, max_be=8, backoff_unit_us=8 * TICK, seed=2)
    d.set_next(d.tree([0]), [0], 0)
    d.inject(list(range(1, nd.n)), 0)
    lists = batch_lists(nd.n)
    tb = [TICK * (b + 1) for b in range(len(lists))]
    if as_batch:
        results = d.batch(tb, [t + TICK for t in tb], lists, [t + 100 for t in tb], AIR)
        for b, res in enumerate(results):
            d.advance(res, slot=b)
    else:
        for b, lst in enumerate(lists):
            d.advance(d.tick(tb[b], tb[b] + TICK, lst, tb[b] + 100, AIR))
    return d


def driver_batch(d, t_begin, t_end, lists, starts, air):
    """the oracle's evaluation of a batch of self-contained ticks: one after the other"""
    return [d.tick(t_begin[b], t_end[b], lists[b], starts[b], air) for b in range(len(lists))]


Driver.batch = driver_batch
