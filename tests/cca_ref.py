"""Expected values of a carrier-sense gated tick from the oracle alone, and the scenes the gated tick's
tests run.  The sensing is tests/energy_ref.py::channel_energy over the frames on the air when the tick begins; the tick is the
oracle's pass over those frames with the kept candidates as its new frames.  No engine code is involved."""
import numpy as np

import energy_ref as R

TICK = 1000
AIR = 8128


class Expected:
    """one tick's heard links with packet numbers counting every slot of the source list (padding and deferred slots included)"""

    def __init__(self, n, slots, res, new):
        self.slots, self.raw, self.new = slots, res, new
        self.count = 0 if res is None else res.count
        z = np.zeros(0)
        self.pkt = slots[res.pkt].astype(np.int32) if res is not None else np.zeros(0, dtype=np.int32)
        self.dst = res.dst if res is not None else np.zeros(0, dtype=np.int32)
        self.verdict = res.verdict if res is not None else np.zeros(0, dtype=np.uint8)
        self.rssi = res.rssi if res is not None else z
        self.sinr = res.sinr if res is not None else z
        self.pkt_interference = res.pkt_interference if res is not None else np.zeros(0, dtype=np.uint8)   # of the slots in `slots`
        self.pkt_offset = np.zeros(n + 1, dtype=np.uint32)
        self.pkt_offset[1:] = np.cumsum(np.bincount(self.pkt, minlength=n))
        self.rng_state = None if res is None else res.rng_state


class Chain:
    """the oracle's view of a run of ticks over the SINR medium: the frames on the air, tick by tick"""

    def __init__(self, O, nd, mdl):
        self.O, self.nd, self.mdl = O, nd, mdl
        self.onair = np.zeros(0, dtype=O.PACKET_DTYPE)

    def expire(self, t_begin):
        self.onair = self.onair[self.onair["start_us"] + self.onair["air_us"] > t_begin]

    def sense(self, src, cca_time, threshold):
        """E5 for every candidate on its own channel over the frames on the air now; padding: flags 0, NaN energy"""
        src = np.asarray(src, dtype=np.int32)
        flags = np.zeros(len(src), dtype=np.uint8)
        energy = np.full(len(src), np.nan)
        ok = np.flatnonzero((src >= 0) & (src < self.nd.n))
        if len(ok):
            energy[ok], flags[ok], _ = R.channel_energy(self.O, self.mdl, self.nd, self.onair, cca_time, nodes=src[ok], threshold=threshold)
        return flags, energy

    def plain_tick(self, t_begin, src, start, air, rng_state=None):
        """what rm_tick_run_sources_device gives for `src` (entries outside 0 .. n-1 are padding)"""
        O = self.O
        self.expire(t_begin)
        src = np.asarray(src, dtype=np.int32)
        slots = np.flatnonzero((src >= 0) & (src < self.nd.n))
        new = self.nd.packets(src[slots], start, air)
        res = None
        if len(slots):
            active = np.concatenate([self.onair, new])
            if rng_state is None:
                res = O.tick_mt(self.mdl, self.nd, active, first_new=len(self.onair), cap=1 << 22)
            else:
                res = O.tick(self.mdl, self.nd, active, first_new=len(self.onair), rng_state=rng_state, cap=1 << 22)
            self.onair = active
        exp = Expected(len(src), slots, res, new)
        if res is None:
            exp.rng_state = rng_state
        return exp

    def gated_tick(self, t_begin, src, start, air, cca_time, threshold, rng_state=None):
        """-> (flags, energy, Expected): sensed before any frame of this call is on the air; deferred candidates become padding"""
        self.expire(t_begin)
        src = np.asarray(src, dtype=np.int32)
        flags, energy = self.sense(src, cca_time, threshold)
        return flags, energy, self.plain_tick(t_begin, np.where(flags != 0, -1, src), start, air, rng_state)


def uniform_nodes(O, n, seed, k=20.0, channels=1):
    rng = np.random.default_rng(seed)
    side = 50.0 * np.sqrt(np.pi * n / k)
    nd = O.NodeTable(n)
    nd.x, nd.y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    if channels > 1:
        nd.channel[:] = 11 + rng.integers(0, channels, n)
    return nd, rng


class Scene:
    """a run of gated ticks: tick k begins at k * TICK, samples at + sample_at, its frames start at + start_at and last AIR"""

    def __init__(self, O, name):
        self.name = name
        if name == "multi":          # several thousand nodes, one channel, shadowing, frames that outlive their tick
            self.nd, rng = uniform_nodes(O, 6000, 41)
            self.params = {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 0xCCA}
            self.n_ticks, per, self.threshold = 12, 150, -88.0
        elif name == "ch16":         # sixteen channels: only co-channel frames are sensed
            self.nd, rng = uniform_nodes(O, 8000, 43, channels=16)
            self.params = {"ld_flags": 1, "ld_sigma_db": 3.0, "ld_seed": 16}
            self.n_ticks, per, self.threshold = 11, 900, -95.0
        else:
            raise KeyError(name)
        self.sample_at, self.start_at = 128, 200
        self.ticks = []
        for k in range(self.n_ticks):
            src = rng.choice(self.nd.n, per, replace=False).astype(np.int32)     # (unsorted: a list is in the caller's order)
            if k % 3 == 1:
                src[rng.choice(per, 5, replace=False)] = -1                      # padding on input
            self.ticks.append(src)

    def times(self, k):
        return k * TICK, k * TICK + self.sample_at, k * TICK + self.start_at

    def model(self, O):
        return O.model(O.MODEL_LOGDIST, **self.params)
