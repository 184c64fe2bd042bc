"""Reference of the frame error model, on top of the untouched oracle: psr() and draw() written
from the spec with the oracle's orc_det_* functions and Python's IEEE doubles (one rounding per operation, no fma), apply()
= the oracle's verdict column after E10.  The library's host exports are never the source of an expected value.
Also the scenes the GPU tests of the model use, so that the CPU tier can hold the REFERENCE ALONE to the conditions that keep
those tests from passing vacuously (tests/test_errmodel_ref.py)."""
import math

import numpy as np

from oracle import oracle as O
from util import oracle_model

GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
BINOM = [float(math.comb(16, k)) for k in range(17)]
NINF = float("-inf")


def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def draw_hash(seed, src, start_us, dst):
    h1 = mix64(mix64((seed + GOLDEN) & M64) ^ (int(start_us) & M64))
    return mix64(h1 ^ (((int(src) & 0xFFFFFFFF) << 32) | (int(dst) & 0xFFFFFFFF)))


def draw(seed, src, start_us, dst):
    return (float(draw_hash(seed, src, start_us, dst) >> 12) + 0.5) * 2.0 ** -52


def ber(sinr_db):
    L = O.lib()
    s = L.orc_det_pow10(sinr_db / 10.0)
    acc = 0.0
    for k in range(2, 17):
        ck = 1.0 / float(k) - 1.0
        yk = ((20.0 * s) * ck) * 1.4426950408889634
        tk = BINOM[k] * L.orc_det_exp2(yk)
        acc = acc + tk if k % 2 == 0 else acc - tk
    b = acc / 30.0
    if b < 0.0:
        b = 0.0
    if 0.5 < b:
        b = 0.5
    return b


def psr(sinr_db, air_us, us_per_bit=4.0):
    L = O.lib()
    b = ber(float(sinr_db))
    if b != b:
        return b
    n = float(int(air_us)) / us_per_bit
    return L.orc_det_exp2(n * L.orc_det_log2(1.0 - b))


def apply_full(new_packets, res, seed=0, us_per_bit=4.0):
    """-> (verdict column after E10, psr per link -- NaN where the link was not RM_DELIVERED before)"""
    verdict = np.array(res.verdict, dtype=np.uint8, copy=True)
    p = np.full(len(verdict), np.nan)
    cache = {}
    for i in np.nonzero(verdict == O.DELIVERED)[0]:
        pk = new_packets[int(res.pkt[i])]
        key = (float(res.sinr[i]).hex(), int(pk["air_us"]))
        if key not in cache:
            cache[key] = psr(float(res.sinr[i]), int(pk["air_us"]), us_per_bit)
        p[i] = cache[key]
        u = draw(seed, int(pk["src"]), int(pk["start_us"]), int(res.dst[i]))
        if not (u < p[i]):
            verdict[i] = O.INTERFERED
    return verdict, p


def apply(active_packets, res, first_new=0, seed=0, us_per_bit=4.0):
    """the verdict column of the oracle's TickResult `res` (over active_packets[first_new:]) after E10"""
    return apply_full(np.atleast_1d(active_packets)[first_new:], res, seed, us_per_bit)[0]


# ---- the scenes of tests/test_gpu_errmodel.py -----------------------------------------------------------------------------
# sensitivity 3 dB below the noise and no capture floor: the links near the sensitivity sit in the curve's transitional region
PARAMS = {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 21, "ld_noise_dbm": -100.0, "ld_sensitivity_dbm": -103.0,
          "ld_capture_db": NINF, "ld_ifloor_dbm": -110.0}
SEED = 77


def nodes(n, k=20.0, seed=1):
    rng = np.random.default_rng(seed)
    side = 50.0 * np.sqrt(np.pi * n / k)
    nd = O.NodeTable(n)
    nd.x, nd.y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    return nd, rng


class Replay:
    """the oracle's view of a run with E10: the frames on the air tick by tick, every tick's result with the model applied"""

    def __init__(self, nd, params=PARAMS, seed=SEED, us_per_bit=4.0):
        self.nd, self.mdl, self.seed, self.upb = nd, oracle_model(O, "logdist", params), seed, us_per_bit
        self.onair = np.zeros(0, dtype=O.PACKET_DTYPE)

    def tick_packets(self, t_begin, new):
        """-> (TickResult with .verdict after E10 and .plain the verdict before it, psr per link)"""
        self.onair = self.onair[self.onair["start_us"] + self.onair["air_us"] > t_begin]
        live = new[new["src"] >= 0]  # (a padding entry is not a frame; packet numbers keep their positions)
        idx = np.nonzero(new["src"] >= 0)[0]
        res = O.tick_mt(self.mdl, self.nd, np.concatenate([self.onair, live]), first_new=len(self.onair), cap=1 << 22)
        res.pkt = idx[res.pkt].astype(np.int32) if len(res.pkt) else res.pkt
        pint = np.zeros(len(new), dtype=np.uint8)
        pint[idx] = res.pkt_interference
        res.pkt_interference = pint
        res.slots = idx  # (the Tx-failure flag of a padding slot is not specified: compared at the live slots, as cca_ref.Expected does)
        res.plain = res.verdict
        res.verdict, p = apply_full(new, res, self.seed, self.upb)
        res.pkt_offset = np.searchsorted(res.pkt, np.arange(len(new) + 1)).astype(np.uint32)
        self.onair = np.concatenate([self.onair, live])
        return res, p

    def tick(self, t_begin, srcs, start, air):
        srcs = np.asarray(srcs, dtype=np.int32)
        new = self.nd.packets(np.where(srcs >= 0, srcs, 0), start, air)
        new["src"] = srcs
        return self.tick_packets(t_begin, new)


def scene_conditions(results):
    """results: [(TickResult from Replay, psr per link)] of one scene -> (transitional, flipped, kept transitional, mixed packets)"""
    trans = flipped = kept = mixed = 0
    for res, p in results:
        was = res.plain == O.DELIVERED
        tr = was & (p > 0.05) & (p < 0.95)
        fl = was & (res.verdict != O.DELIVERED)
        trans += int(tr.sum())
        flipped += int(fl.sum())
        kept += int((tr & ~fl).sum())
        for q in np.unique(res.pkt[fl]):
            if ((res.pkt == q) & was & ~fl).any():
                mixed += 1
    return trans, flipped, kept, mixed


TICK = 1000


def scene_lone():
    """one tick, 60 frames that all start at 0 (they interfere with each other): -> nd, srcs, start, air"""
    nd, rng = nodes(1500)
    return nd, np.sort(rng.choice(nd.n, 60, replace=False)).astype(np.int32), 0, 4064


def scene_serial():
    """30 frames one after the other (none overlaps another: rm_transmit packet by packet sees what one tick sees):
    -> nd, srcs, starts, hex_length, air"""
    nd, rng = nodes(1500, seed=2)
    srcs = rng.choice(nd.n, 30, replace=False).astype(np.int32)
    hex_len = 254  # 127 bytes
    air = int(O.lib().orc_air_time_us(hex_len))
    return nd, srcs, np.arange(30, dtype=np.int64) * (air + 500), hex_len, air


def scene_batch(overlap):
    """six ticks: an empty list, padding entries, a link count that is no multiple of 64, one slot above 16 384 links.
    overlap: 8128 us frames over 1000 us ticks, else 640 us frames (self-contained): -> nd, lists, starts, air"""
    nd, rng = nodes(3000, seed=3 if overlap else 4)
    sizes = [40, 0, 48, 150, 33, 20]
    lists = [np.sort(rng.choice(nd.n, s, replace=False)).astype(np.int32) for s in sizes]
    lists[2][[0, 7, 47]] = -1
    return nd, lists, [k * TICK for k in range(len(sizes))], 8128 if overlap else 640
