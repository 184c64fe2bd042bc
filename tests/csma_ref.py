"""Expected values of a CSMA-CA gated batch from the oracle alone: a Python restatement of mix64, the backoff
draw and the schedule, and a run that goes tick by tick through tests/cca_ref.py::Chain -- expire, sense over the made entries, the
first-wins rule in Python, plain_tick over the kept list -- with the packets' status, attempts, tick, pkt, flags and energy.  No engine
code is involved."""
import numpy as np

import cca_batch_ref as BR
import cca_ref as CR
import energy_ref as R

NONE, SENT, FAILED, PENDING = 0, 1, 2, 3
TRYING = 255
M64 = (1 << 64) - 1
_CACHE = {}


class Params:
    def __init__(self, max_backoffs=4, min_be=3, max_be=5, seed=0):
        self.max_backoffs, self.min_be, self.max_be, self.seed = max_backoffs, min_be, max_be, seed

    def key(self):
        return (self.max_backoffs, self.min_be, self.max_be, self.seed)


def mix64(z):
    """E2's SplitMix64 finaliser"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def backoff(p, t_cca_origin, k, a):
    """ticks between attempt a and attempt a + 1 of the packet in slot k of the tick sampled at t_cca_origin, minus one"""
    be = min(p.min_be + a, p.max_be)
    if be == 0:
        return 0
    h1 = mix64(mix64(p.seed + 0x9E3779B97F4A7C15) ^ (t_cca_origin & M64))
    h2 = mix64(h1 ^ ((k << 8) | a))
    return h2 >> (64 - be)


def schedule(p, n_src, t_cca):
    """-> per tick the expanded list as [(packet, attempt, tick of the next attempt or -1)], own entries first, then the retries ordered
    by (origin tick, origin slot); packet: the flat index over the own lists"""
    n_ticks = len(n_src)
    first = np.concatenate([[0], np.cumsum(n_src)]).astype(np.int64)
    retries = [[] for _ in range(n_ticks)]
    own = [[] for _ in range(n_ticks)]
    for b in range(n_ticks):
        for k in range(int(n_src[b])):
            o, tick = int(first[b]) + k, b
            for a in range(p.max_backoffs + 1):
                nxt = tick + 1 + backoff(p, int(t_cca[b]), k, a) if a < p.max_backoffs else -1
                (own[b] if a == 0 else retries[tick]).append((o, a, nxt))
                if nxt < 0 or nxt >= n_ticks:
                    break
                tick = nxt
    out = []
    for b in range(n_ticks):
        assert retries[b] == sorted(retries[b])            # (origin tick, origin slot) is the order of the flat packet index
        out.append(own[b] + retries[b])
    return out


class Run:
    """a CSMA-CA gated batch over `lists` on the scene's clock, through the oracle's chain.  first_wins=False and phantom=True are the
    two WRONG readings the tests hold the scenes against: "a sibling is kept too", and "a deferred packet's later attempts are sensed
    as if its deferred frames were on the air"."""

    def __init__(self, O, sc, lists, p, threshold=None, air=CR.AIR, first_wins=True, phantom=False, chain=None, first_tick=0):
        nd = sc.nd
        self.lists = [np.asarray(s, dtype=np.int32) for s in lists]
        n_ticks = len(self.lists)
        thr = sc.threshold if threshold is None else threshold
        times = [sc.times(first_tick + b) for b in range(n_ticks)]
        self.sched = schedule(p, [len(s) for s in self.lists], [t[1] for t in times])
        self.n_exp = np.array([len(s) for s in self.sched], dtype=np.int32)
        entries = np.concatenate(self.lists + [np.zeros(0, dtype=np.int32)])
        n_pkt = len(entries)
        self.status = np.full(n_pkt, TRYING, dtype=np.uint8)
        self.attempts = np.zeros(n_pkt, dtype=np.uint8)
        self.tick = np.full(n_pkt, -1, dtype=np.int32)
        self.pkt = np.full(n_pkt, -1, dtype=np.int32)
        self.flags = np.zeros(n_pkt, dtype=np.uint8)
        self.energy = np.full(n_pkt, np.nan)
        self.status[(entries < 0) | (entries >= nd.n)] = NONE
        chain = CR.Chain(O, nd, sc.model(O)) if chain is None else chain
        ghosts = np.zeros(0, dtype=O.PACKET_DTYPE)
        self.made, self.kept, self.slot_flags, self.slot_energy, self.exp, self.onair = [], [], [], [], [], []
        self.sibling_losses = 0
        for T in range(n_ticks):
            t0, tc, ts = times[T]
            chain.expire(t0)
            slots = self.sched[T]
            node = np.array([entries[o] for o, _, _ in slots], dtype=np.int32).reshape(-1)
            made = np.array([0 <= entries[o] < nd.n and (a == 0 or self.status[o] == TRYING) for o, a, _ in slots], dtype=bool).reshape(-1)
            made_list = np.where(made, node, -1).astype(np.int32)
            if phantom:
                real = chain.onair
                chain.onair = np.concatenate([real, ghosts])
                flags, energy = chain.sense(made_list, tc, thr)
                chain.onair = real
            else:
                flags, energy = chain.sense(made_list, tc, thr)
            keep = np.zeros(len(slots), dtype=bool)
            winners = set()
            for i in np.flatnonzero(made & (flags == 0)):          # one frame per radio per tick: the first in list order wins
                if first_wins and int(node[i]) in winners:
                    flags[i] |= R.ED_TRANSMITTING
                    self.sibling_losses += 1
                else:
                    keep[i] = True
                    winners.add(int(node[i]))
            kept_list = np.where(keep, node, -1).astype(np.int32)
            exp = chain.plain_tick(t0, kept_list, ts, air)
            if phantom:
                lost = made & ~keep
                ghosts = np.concatenate([ghosts[ghosts["start_us"] + ghosts["air_us"] > t0], nd.packets(node[lost], ts, air)])
            for i, (o, a, nxt) in enumerate(slots):
                if not made[i]:
                    continue
                self.attempts[o], self.flags[o], self.energy[o] = a + 1, flags[i], energy[i]
                if keep[i]:
                    self.status[o], self.tick[o], self.pkt[o] = SENT, T, i
                elif nxt < 0:
                    self.status[o] = FAILED
                elif nxt >= n_ticks:
                    self.status[o], self.tick[o] = PENDING, nxt
            self.made.append(made_list)
            self.kept.append(kept_list)
            self.slot_flags.append(flags)
            self.slot_energy.append(energy)
            self.exp.append(exp)
            self.onair.append(chain.onair.copy())
        assert not (self.status == TRYING).any()

    def outcome(self):
        return np.stack([self.status.astype(np.int64), self.attempts.astype(np.int64), self.tick.astype(np.int64), self.pkt.astype(np.int64),
                         self.flags.astype(np.int64)])


# the scenes of the issue's table: (scene, ticks, parameters)
SCENES = {"multi": (12, Params(4, 1, 3, 7)), "ch16": (11, Params(3, 1, 2, 9))}


def run(O, name, **kw):
    """a scene's run with its table parameters, computed once and left unchanged (kw: a wrong reading)"""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        sc = BR.scene(O, name)
        ticks, p = SCENES[name]
        _CACHE[key] = Run(O, sc, sc.ticks[:ticks], p, **kw)
    return _CACHE[key]


class ChainRun:
    """cca_batch_ref.ChainScene's A, B, C with frames of 960 us (shorter than a tick, still on the air at the next tick's sample, gone
    at the one after), every retry in the next tick (min_be = max_be = 0), max_backoffs = 2: A in tick 0, B in tick 1, C in tick 2, A
    in tick 3, each after the scene's own candidates of that tick."""
    AIR = 960

    def __init__(self, O):
        sc = BR.scene(O, "chain")
        base = BR.scene(O, "multi")
        self.sc, self.p = sc, Params(2, 0, 0, 1)
        extra = (sc.a, sc.b, sc.c, sc.a)
        self.lists = [np.concatenate([base.ticks[k], np.array([extra[k]], dtype=np.int32)]) for k in range(4)]
        self.first = np.concatenate([[0], np.cumsum([len(s) for s in self.lists])])
        self.at = [int(self.first[k]) + len(self.lists[k]) - 1 for k in range(4)]     # the packets of A, B, C, A
        self.run = Run(O, sc, self.lists, self.p, air=self.AIR)


def chain_run(O):
    if "chain" not in _CACHE:
        _CACHE["chain"] = ChainRun(O)
    return _CACHE["chain"]
