"""A host model of the reception stage's two rings (radio-sim_amd/csrc/rm_events.hip: the pending packets and their heard links,
each a power of two long), and the CPU side of the sessions that wrap, fill and overflow them.

The model needs nothing but packet times and per-packet link counts, which come from the oracle's tick; no engine code is involved
and the library is never the source of an expected value.  The rule (include/radiomedium_hip.h at rm_events_enable):

  hand-over of a tick of n_new records (padding records included) with L heard links at current time `now`:
    the tick is dropped if (tail - head) + n_new > packet capacity or (pool_tail - pool_head) + L > link capacity; a dropped tick
    keeps its packet numbers but stores nothing, and the next drain reports it, once; otherwise packet q is stored with
    t0 = max(start, now), t1 = t0 + air and link_off = the running link offset.
  drain(T):
    head moves to the first packet of the ring (this tick's included) that was not finished BEFORE this drain, or to tail;
    pool_head becomes that packet's link_off, or pool_tail; then every packet with t1 < T is finished (a packet of the
    constant-loss medium by the first drain after its hand-over, whatever its times; a padding record as it is stored).
    pending_packets = tail - head after the move, oldest_packet = the head packet's number, or the next number if the ring
    is empty.

Traffic is what tests/test_gpu_events_batch.py's Session does without an engine: the seeded ticks, the oracle's evaluation of them,
the oracle's serial event replay (oracle.Sim) and, where capacities are given, this model.  Session adds the engine on top, so
tests/test_events_ring_ref.py (no GPU) and tests/test_gpu_events_rings.py walk the same ticks; the former holds the scenes'
conditions -- wraps, straddling packets, drops, exact fits, group counts -- so that no GPU test passes vacuously."""
import numpy as np

from util import oracle_model, random_nodes

MIN_CAP = 64


def pow2_at_least(v):
    p = MIN_CAP
    while p < v:
        p <<= 1
    return p


class Rings:
    def __init__(self, pk_cap, pool_cap):
        self.pk_cap, self.pool_cap = pow2_at_least(pk_cap), pow2_at_least(pool_cap)
        self.head = self.tail = self.pool_head = self.pool_tail = 0
        self.next_packet = 0
        self.ring = []                # [number, t0, t1, link_off, link_cnt, start fired, finished, immediate] of head .. tail
        self.err = False              # a dropped tick the next drain reports
        self.ticks = 0
        self.dropped = []             # (tick number, "packets" / "links" / "both")
        self.max_packets = self.max_links = 0
        self.exact_fit = {"packets": 0, "links": 0}
        self.straddles = 0
        self.reports = 0

    def hand_over(self, now, start_us, air_us, link_cnt, immediate=False, padding=None):
        """one evaluated tick; -> kept?"""
        n_new = len(start_us)
        tick = self.ticks
        self.ticks += 1
        if n_new == 0:                # (no hand-over at all)
            return True
        link_cnt = np.asarray(link_cnt, dtype=np.int64)
        total = int(link_cnt.sum())
        no_pk = (self.tail - self.head) + n_new > self.pk_cap
        no_pool = (self.pool_tail - self.pool_head) + total > self.pool_cap
        first = self.next_packet
        self.next_packet += n_new     # the packets were transmitted, kept or not
        if no_pk or no_pool:
            self.err = True
            self.dropped.append((tick, "both" if no_pk and no_pool else "packets" if no_pk else "links"))
            return False
        off = self.pool_tail
        for q in range(n_new):
            t0 = max(int(start_us[q]), int(now))
            pad = padding is not None and bool(padding[q])       # no packet: finished as it is stored
            cnt = int(link_cnt[q])
            self.ring.append([first + q, t0, t0 + int(air_us[q]), off, cnt, pad or bool(immediate), pad, bool(immediate)])
            if cnt and (off % self.pool_cap) + cnt > self.pool_cap:
                self.straddles += 1
            off += cnt
        self.tail += n_new
        self.pool_tail = off
        self.max_packets = max(self.max_packets, self.tail - self.head)
        self.max_links = max(self.max_links, self.pool_tail - self.pool_head)
        self.exact_fit["packets"] += (self.tail - self.head) == self.pk_cap
        self.exact_fit["links"] += (self.pool_tail - self.pool_head) == self.pool_cap
        return True

    def drain(self, T):
        """-> (pending_packets, oldest_packet, does this drain report a dropped tick, fired (packet, flank) groups)"""
        live = next((i for i, p in enumerate(self.ring) if not p[6]), len(self.ring))
        del self.ring[:live]
        self.head += live
        self.pool_head = self.ring[0][3] if self.ring else self.pool_tail
        groups = 0
        for p in self.ring:
            if p[6]:
                continue
            if not p[5] and p[1] < T:
                p[5] = True
                groups += 1
            if p[7] or p[2] < T:      # (the constant-loss medium's packet: delivered by the first drain, whatever its times)
                p[6] = True
                groups += 1
        reported, self.err = self.err, False
        self.reports += reported
        return self.tail - self.head, (self.ring[0][0] if self.ring else self.next_packet), reported, groups

    def report(self):
        return dict(dropped=list(self.dropped), max_packets=self.max_packets, max_links=self.max_links,
                    packet_wraps=self.tail / self.pk_cap, link_wraps=self.pool_tail / self.pool_cap, straddles=self.straddles,
                    exact_fit=dict(self.exact_fit))


class Traffic:
    """The CPU side of one reception-stage session: seeded ticks, the oracle's evaluation and serial event replay, and the ring
    model where `capacity` = (packets, links) is given.  lone / batch / drain here only move the oracle's side on; Session
    (tests/test_gpu_events_batch.py) overrides them with the engine's calls and the comparison."""

    def __init__(self, O, seed, kind, params, n=1500, per_tick=30, tick_styles=(1000,), aligned=False, hex_lengths=(0, 2, 20, 64, 254),
                 matrix=None, sinr=False, own=None, draws=True, min_per_tick=0, capacity=None, by_sources=False):
        self.O, self.kind, self.own, self.sinr = O, kind, own, sinr
        self.by_sources = by_sources or sinr      # ticks named by source indices: one start and one air time per tick
        self.rng = rng = np.random.default_rng(seed)
        self.n, self.per_tick, self.tick_styles, self.aligned, self.hex_lengths = n, per_tick, tick_styles, aligned, hex_lengths
        self.min_per_tick = min_per_tick
        side = 50.0 * np.sqrt(np.pi * n / 20.0)
        self.nodes = nodes = random_nodes(O, n, side, seed)
        if draws:
            nodes.rxprob[rng.choice(n, n // 5, replace=False)] = 0.6
            nodes.txprob[rng.choice(n, n // 20, replace=False)] = 0.5
        nodes.enabled[rng.choice(n, n // 50, replace=False)] = 0
        self.mdl = oracle_model(O, kind, params, matrix)
        self.state = O.lib().orc_jrandom_seed(seed)
        self.sim = O.Sim(n)
        self.now, self.base, self.delivered = 0, 0, 0
        self.onair = np.zeros(0, dtype=O.PACKET_DTYPE)
        self.capacity = capacity
        self.rings = Rings(*capacity) if capacity is not None else None
        self.kept = []                # per tick: did the rings take it (always, without the model)

    def _packets(self, t_end):
        rng, n = self.rng, self.n
        t = int(rng.integers(self.min_per_tick, self.per_tick + 1))
        src = np.sort(rng.choice(n, t, replace=False)).astype(np.int32)
        if self.by_sources:   # one start, one air time per tick (the frames are named by source indices)
            return src, self.nodes.packets(src, self.now, 32 * int(rng.choice(self.hex_lengths)))
        pk = self.nodes.packets(src, 0, 0)
        pk["start_us"] = self.now if self.aligned else rng.integers(self.now - 50, t_end, t)   # a start before "now" is clamped
        pk["air_us"] = 32 * rng.choice(self.hex_lengths, t)
        return src, pk

    def _next_tick(self):
        t_end = self.now + int(self.rng.choice(self.tick_styles))
        src, pk = self._packets(t_end)
        return t_end, src, pk

    def _oracle_tick(self, pk):
        """the oracle's evaluation of the tick at self.now, handed to its event replay -- unless the rings refuse the tick: it is
        evaluated all the same (the generator moves on) and numbered, but leaves no events"""
        O = self.O
        if self.sinr:
            self.onair = self.onair[self.onair["start_us"] + self.onair["air_us"] > self.now]
            want = O.tick(self.mdl, self.nodes, np.concatenate([self.onair, pk]), first_new=len(self.onair), rng_state=self.state)
            self.onair = np.concatenate([self.onair, pk])
        else:
            want = O.tick(self.mdl, self.nodes, pk, rng_state=self.state)
        self.state = want.rng_state
        const = self.kind == "udgm_const"
        kept = True
        if self.rings is not None:
            kept = self.rings.hand_over(self.now, pk["start_us"], pk["air_us"], np.bincount(want.pkt, minlength=len(pk)),
                                        immediate=const, padding=pk["src"] < 0)
        self.kept.append(kept)
        imm = self.sim.medium_calls(want, pk, pkt_base=self.base, const_loss=const) if kept else []
        self.base += len(pk)
        return imm

    def _model_drain(self, t):
        """-> (pending_packets, oldest_packet, reports a dropped tick) of the drain at t, or None without the model"""
        return self.rings.drain(t)[:3] if self.rings is not None else None

    # ---- the steps of a plan (run_plan), oracle side only
    def lone(self, what):
        t_end, _, pk = self._next_tick()
        imm = self._oracle_tick(pk)
        self.drain(t_end, what, imm)

    def batch(self, k, what):
        for b in range(k):
            self.lone("%s batch tick %d" % (what, b))

    def drain(self, t, what, imm=()):
        ev = self.sim.step(t)
        self.delivered += int((ev["kind"] == self.O.EV_RX_END_DELIVERY).sum()) + len(imm)
        self._model_drain(t)
        self.now = t

    def finish(self):
        self.drain(self.now + 10 ** 7, "final drain")
        assert self.sim.pending == 0
        if self.rings is not None:
            assert self.rings.drain(self.now + 1)[:2] == (0, self.base)
        self.sim.close()
        return self.delivered


# ---------------------------------------------------------------- the scenes
HEX = (0, 2, 20, 64, 127)
LONE_PLAN = ("lone",) * 120
MIXED_PLAN = (7, "lone", 1, 64, "drain", "lone", 7, 3, "drain", 1, 20, "lone", 14)    # 120 ticks; one batch of 64


def plan_ticks(plan):
    return sum(1 if s == "lone" else 0 if s == "drain" else int(s) for s in plan)


# name -> (seed, medium, parameters, Traffic keywords); every wrap session has 120 ticks.  (The SINR scene hands in up to 7 frames
# per tick: with up to 5, sixteen seeds in a row passed 2.2 - 2.8 link capacities through the link ring, never three.)
WRAP = {
    "udgm_draws": (1103, "udgm", dict(udgm_success_ratio_rx=0.8),
                   dict(n=300, per_tick=8, tick_styles=(1000, 1000, 10, 3000), hex_lengths=HEX, capacity=(64, 2048))),
    "aligned": (1200, "udgm", {}, dict(n=300, per_tick=8, aligned=True, hex_lengths=(62,), capacity=(64, 2048))),
    "logdist": (1302, "logdist", dict(ld_sigma_db=4.0, ld_seed=77), dict(n=300, per_tick=8, hex_lengths=HEX, capacity=(64, 4096))),
    "null": (1401, "null", {}, dict(n=150, per_tick=4, hex_lengths=HEX, capacity=(64, 4096))),
    "const": (1500, "udgm_const", {}, dict(n=300, per_tick=8, hex_lengths=HEX, capacity=(64, 4096))),
    # the first scene with its ticks named by source indices (rm_tick_run_sources_device): the only lone tick whose append waits for
    # the drain and rides in its first launch (k_ev_append_select)
    "udgm_sources": (1701, "udgm", dict(udgm_success_ratio_rx=0.8),
                     dict(n=300, per_tick=8, tick_styles=(1000, 1000, 10, 3000), hex_lengths=HEX, by_sources=True, capacity=(64, 2048))),
    "sinr": (1603, "logdist", dict(ld_flags=1, ld_sigma_db=4.0, ld_seed=5),
             dict(n=300, per_tick=7, hex_lengths=(10, 64, 127), sinr=True, draws=False, capacity=(64, 4096))),
}
# the ring that refuses ticks (_sources: the ticks named by source indices) -> (seed, medium, parameters, Traffic keywords); 60 lone ticks
OVERFLOW_TICKS = 60
OVERFLOW = {
    "packets": (2104, "udgm", dict(udgm_success_ratio_rx=0.8),
                dict(n=300, per_tick=14, hex_lengths=(20, 64, 254, 254), capacity=(64, 1 << 14))),
    "packets_sources": (2303, "udgm", dict(udgm_success_ratio_rx=0.8),
                        dict(n=300, per_tick=14, hex_lengths=(20, 64, 254, 254), by_sources=True, capacity=(64, 1 << 14))),
    "links": (2206, "udgm", dict(udgm_success_ratio_rx=0.8), dict(n=300, per_tick=8, hex_lengths=(20, 64, 127), capacity=(1024, 512))),
}


def wrap_traffic(O, name):
    seed, kind, params, kw = WRAP[name]
    return Traffic(O, seed, kind, params, **kw)


def overflow_traffic(O, name):
    seed, kind, params, kw = OVERFLOW[name]
    return Traffic(O, seed, kind, params, **kw)


def wrap_conditions(rep, what):
    """what every wrap scene must do to its rings for the comparison with the engine to mean anything"""
    assert not rep["dropped"], "%s: dropped ticks %s" % (what, rep["dropped"])
    assert rep["packet_wraps"] >= 3, "%s: the packet ring wrapped %.1f times" % (what, rep["packet_wraps"])
    assert rep["link_wraps"] >= 3, "%s: the link ring wrapped %.1f times" % (what, rep["link_wraps"])
    assert rep["straddles"] >= 2, "%s: %d packets straddle the pool's end" % (what, rep["straddles"])


def overflow_conditions(rep, name, what):
    name = name.split("_")[0]
    rings = {r for _, r in rep["dropped"]}
    assert rings == {name}, "%s: ticks refused by %s" % (what, sorted(rings))
    assert 2 <= len(rep["dropped"]) <= OVERFLOW_TICKS // 2, "%s: %d ticks dropped" % (what, len(rep["dropped"]))
    assert rep["exact_fit"][name] >= 1, "%s: no accepted tick filled the ring exactly (maximum %d / %d)" % (
        what, rep["max_packets"], rep["max_links"])


# ---------------------------------------------------------------- more than 2048 groups in one drain
GROUPS_CAPACITY = (4096, 1 << 17)
GROUPS_P = (1024, 1025)          # 2 P groups: the LDS key staging of k_ev_emit exactly full / the rank pass from global memory
GROUPS_AIR_US = 10 ** 6
GROUPS_PER_TICK = 35


def groups_script(O, P, seed=3100, n=300):
    """P packets of a second's air time handed in over ~30 ticks of 1000 us, every start behind the last tick's end: the drains
    at the tick ends fire nothing (the queue's ladder rule moves all the same), the one after them fires every start and every
    end -- 2 P groups.  -> (nodes, [(begin, end, packets)], the last drain's time)"""
    rng = np.random.default_rng(seed)
    nodes = random_nodes(O, n, 50.0 * np.sqrt(np.pi * n / 20.0), seed)
    nodes.enabled[rng.choice(n, n // 50, replace=False)] = 0
    n_ticks = -(-P // GROUPS_PER_TICK)
    first_start = 1000 * n_ticks + 500
    ticks, left = [], P
    for k in range(n_ticks):
        t = min(GROUPS_PER_TICK, left)
        left -= t
        src = np.sort(rng.choice(n, t, replace=False)).astype(np.int32)
        pk = nodes.packets(src, 0, GROUPS_AIR_US)
        pk["start_us"] = first_start + rng.integers(0, 1000, t)     # (starts and ends tie now and then)
        ticks.append((1000 * k, 1000 * (k + 1), pk))
    return nodes, ticks, first_start + 1000 + GROUPS_AIR_US + 1
