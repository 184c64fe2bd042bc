"""The link estimator as a reference: the fold rule in Python integers over numpy tables, and scenes --
sequences of input tables (a watch table and a forwarding table) with the mutations between folds that the rule has a case for.
The record layouts are written out here, not taken from the package: a disagreement about a layout fails the comparison."""
import collections

import numpy as np

M64 = (1 << 64) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)

LINK_STATS = np.dtype([("heard", "<u8"), ("delivered", "<u8"), ("rssi_q8_sum", "<i8"), ("sinr_q8_sum", "<i8"), ("first_start_us", "<i8"),
                       ("last_start_us", "<i8")])
ENTRY = np.dtype([("base_heard", "<u8"), ("base_delivered", "<u8"), ("etx", "<u4"), ("windows", "<u4"), ("data_windows", "<u4"), ("peer", "<i4")])
NODE = np.dtype([("base_tx", "<u8"), ("base_ack", "<u8"), ("base_next", "<i4"), ("data_samples", "<u4"), ("data_unmatched", "<u4"),
                 ("restarted", "<u4")])
FWD_NODE = np.dtype([(f, "<u8") for f in ("generated", "arrived", "lost", "latency_us_sum", "latency_us_max", "hops_sum", "attempts", "acked",
                                          "failed", "deferred", "rejected", "dropped")] +
                    [("ready_us", "<i8"), ("next", "<i4"), ("queue_len", "<i4"), ("queue_max", "<i4"), ("tries", "<i4"), ("slot_mask", "<u4"),
                     ("reserved", "<u4")])
TOTALS = ("folds", "beacon_samples", "data_samples", "data_unmatched", "restarted", "cleared", "estimates", "reserved")
assert LINK_STATS.itemsize == 48 and ENTRY.itemsize == 32 and NODE.itemsize == 32 and FWD_NODE.itemsize == 128

DEFAULTS = dict(beacon_window=3, data_window=5, beacon_alpha_q8=230, data_alpha_q8=230, max_etx=6400)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def valid(p):
    return (0 <= p["beacon_window"] <= 1 << 31 and 0 <= p["data_window"] <= 1 << 31 and 0 <= p["beacon_alpha_q8"] <= 255 and
            0 <= p["data_alpha_q8"] <= 255 and 128 <= p["max_etx"] <= 65535 and p.get("reserved", 0) == 0)


def etx_ratio(heard, delivered):
    """E21's quotient in uint64 arithmetic (modulo 2^64), delivered >= 1"""
    return max(128, ((128 * heard + (delivered >> 1)) & M64) // delivered)


def entry_cost(min_heard, max_link_cost, heard, delivered):
    """E21's inbound cost of an entry, or None when it does not count"""
    if heard < max(min_heard, 1) or heard > 1 << 40 or delivered < 1:
        return None
    q = etx_ratio(heard, delivered)
    return None if q > max_link_cost else q


def ewma(a, old, s):
    return s if old == 0 else (a * old + (256 - a) * s + 128) >> 8


def sample(max_etx, dn, dd):
    return max_etx if dd == 0 else min(max_etx, etx_ratio(dn, dd))


def cleared_stats(shape):
    s = np.zeros(shape, dtype=LINK_STATS)
    s["first_start_us"] = I64_MAX
    s["last_start_us"] = I64_MIN
    return s


class Ref:
    """the estimator's five tables and the fold over them"""

    def __init__(self, n, K, p):
        assert valid(p) and K in (1, 2, 4, 8)
        self.n, self.K, self.p = n, K, dict(p)
        self.log = collections.Counter()
        self.reset()

    def reset(self):
        n, K = self.n, self.K
        self.entry = np.zeros((n, K), dtype=ENTRY)
        self.entry["peer"] = -1
        self.node = np.zeros(n, dtype=NODE)
        self.node["base_next"] = -1
        self.pub_peer = np.full((n, K), -1, dtype=np.int32)
        self.pub_stats = cleared_stats((n, K))
        self.tot = dict.fromkeys(TOTALS, 0)

    def totals(self):
        return dict(self.tot)

    def _publish(self, j, k):
        e = self.entry[j, k]
        self.pub_peer[j, k] = e["peer"]
        s = self.pub_stats[j, k]
        etx = int(e["etx"])
        s["heard"], s["delivered"] = (etx, 128) if etx else (0, 0)
        s["rssi_q8_sum"] = s["sinr_q8_sum"] = 0
        s["first_start_us"], s["last_start_us"] = I64_MAX, I64_MIN

    def fold(self, peer, stats, fwd=None):
        """peer int32 [n][K], stats LINK_STATS [n][K], fwd FWD_NODE [n] or None; none of them is written"""
        n, K, p, tot, log = self.n, self.K, self.p, self.tot, self.log
        assert peer.shape == (n, K) and stats.shape == (n, K) and (fwd is None or fwd.shape == (n,))
        tot["folds"] += 1
        for j in range(n):
            before = [(int(self.entry[j, k]["etx"]), int(self.entry[j, k]["peer"])) for k in range(K)]
            for k in range(K):
                e = self.entry[j, k]
                q, H, D = int(peer[j, k]), int(stats[j, k]["heard"]), int(stats[j, k]["delivered"])
                if q < 0 or q >= n or q == j:
                    if int(e["peer"]) != -1:
                        tot["cleared"] += 1
                    self.entry[j, k] = (0, 0, 0, 0, 0, -1)
                    continue
                if q != int(e["peer"]) or H < int(e["base_heard"]) or D < int(e["base_delivered"]):
                    self.entry[j, k] = (0, 0, 0, 0, 0, q)
                    tot["restarted"] += 1
                    self.node[j]["restarted"] += 1
                dH, dD = H - int(e["base_heard"]), D - int(e["base_delivered"])
                if p["beacon_window"] > 0 and dH >= p["beacon_window"]:
                    e["etx"] = ewma(p["beacon_alpha_q8"], int(e["etx"]), sample(p["max_etx"], dH, dD))
                    e["windows"] += 1
                    e["base_heard"], e["base_delivered"] = H, D
                    tot["beacon_samples"] += 1
                    log["zero_delivered"] += dD == 0
                elif p["beacon_window"] > 0 and dH > 0:
                    log["partial"] += 1
            if fwd is not None and p["data_window"] > 0:
                nd = self.node[j]
                w, A = int(fwd[j]["next"]), int(fwd[j]["acked"])
                T = (A + int(fwd[j]["failed"])) & M64
                if w != int(nd["base_next"]) or T < int(nd["base_tx"]) or A < int(nd["base_ack"]):
                    nd["base_next"], nd["base_tx"], nd["base_ack"] = w, T, A
                    log["rebased"] += 1
                elif 0 <= w < n and w != j and T - int(nd["base_tx"]) >= p["data_window"]:
                    dT, dA = T - int(nd["base_tx"]), A - int(nd["base_ack"])
                    nd["base_tx"], nd["base_ack"] = T, A
                    slots = [k for k in range(K) if int(self.entry[j, k]["peer"]) == w]
                    if not slots:
                        nd["data_unmatched"] += 1
                        tot["data_unmatched"] += 1
                    else:
                        e = self.entry[j, slots[0]]
                        e["etx"] = ewma(p["data_alpha_q8"], int(e["etx"]), sample(p["max_etx"], dT, dA))
                        e["data_windows"] += 1
                        nd["data_samples"] += 1
                        tot["data_samples"] += 1
                        log["data_dup_row"] += len(slots) > 1
            for k in range(K):
                etx, q = int(self.entry[j, k]["etx"]), int(self.entry[j, k]["peer"])
                tot["estimates"] += (etx != 0) - (before[k][0] != 0)
                if (etx, q) != before[k]:
                    self._publish(j, k)
        log["between_seen"] += self.between() > 0

    def between(self):
        """entries whose estimate lies strictly between 128 and max_etx"""
        etx = self.entry["etx"]
        return int(((etx > 128) & (etx < self.p["max_etx"])).sum())


def same(ref, entry, node, pub_peer, pub_stats, totals, what):
    """every table against the reference, bit for bit"""
    assert entry.tobytes() == ref.entry.tobytes(), what + ": entries"
    assert node.tobytes() == ref.node.tobytes(), what + ": node state"
    assert np.asarray(pub_peer, dtype=np.int32).tobytes() == ref.pub_peer.tobytes(), what + ": published peers"
    assert pub_stats.tobytes() == ref.pub_stats.tobytes(), what + ": published entries"
    assert totals == ref.totals(), (what, totals, ref.totals())


# ---- scenes: the inputs of a sequence of folds ---------------------------------------------------------------------------------------

FOLDS = 20
# node 0's script (it exists in every table of two or more nodes, its slot 0 watches node 1 and its next hop is node 1):
#  folds 0 .. 9   heard +2 per fold against beacon_window 3 -- every other fold the window is not yet full --, delivered +1 per fold
#                 but none in folds 4 .. 5 (a window without a delivery); acked +2 and failed +1 per fold: a data sample every
#                 other fold
#  fold 10        the counters back to 0 (rm_linkstats_reset): a restart
#  folds 14 .. 16 the slot emptied: cleared, and the data sample that falls due finds no slot
#  fold 17 ..     the peer back: a restart
RESET_AT, EMPTY_FROM, EMPTY_TO = 10, 14, 16


def scene(n, K, seed=1, folds=FOLDS):
    """-> a list of (peer, stats, fwd) per fold.  Node 0 follows the script above; every other row moves at random, with a peer
    change, counters reset to 0, a changed next hop, forwarding counters reset, emptied slots (-1, the node itself, an index at or
    above n), duplicate peers in a row, a next hop that no slot holds, delivered > heard and counters near 2^40 among its moves."""
    rng = np.random.default_rng(seed * 1000 + n * 8 + K)
    peer = np.full((n, K), -1, dtype=np.int32)
    stats = cleared_stats((n, K))
    fwd = np.zeros(n, dtype=FWD_NODE)
    fwd["next"] = -1
    prr = rng.choice([0.0, 0.3, 0.6, 0.9, 1.0], size=(n, K))          # (0.0: an entry that never delivers)

    def pick(j):
        r = rng.integers(0, 10)
        return [-1, j, n + int(rng.integers(0, 5))][r] if r < 3 else int(rng.integers(0, n))
    for j in range(n):
        for k in range(K):
            peer[j, k] = pick(j)
            if rng.integers(0, 6) == 0:                               # (a long-running counter)
                stats[j, k]["heard"] = (1 << 40) - int(rng.integers(0, 40))
                stats[j, k]["delivered"] = int(stats[j, k]["heard"]) - int(rng.integers(0, 1 << 20))
        if K > 1 and j % 3 == 1:
            peer[j, K - 1] = peer[j, 0]                               # (a duplicate peer)
        fwd[j]["next"] = int(peer[j, int(rng.integers(0, K))]) if rng.integers(0, 4) else [-2, -1, (j + 1) % n, j][int(rng.integers(0, 4))]
    out = []
    for f in range(folds):
        for j in range(n):
            for k in range(K):
                dh = int(rng.integers(0, 5))
                dd = int(rng.binomial(dh, prr[j, k])) + (2 if rng.integers(0, 40) == 0 else 0)   # (now and then delivered > heard)
                stats[j, k]["heard"] = int(stats[j, k]["heard"]) + dh
                stats[j, k]["delivered"] = int(stats[j, k]["delivered"]) + dd
                m = int(rng.integers(0, 60))
                if m == 0:
                    peer[j, k] = pick(j)
                elif m == 1:
                    stats[j, k]["heard"] = stats[j, k]["delivered"] = 0
                elif m == 2 and K > 1:
                    peer[j, k] = peer[j, (k + 1) % K]
            for name, top in (("acked", 4), ("failed", 3), ("deferred", 3)):
                fwd[j][name] = int(fwd[j][name]) + int(rng.integers(0, top))
            fwd[j]["attempts"] = int(fwd[j]["acked"]) + int(fwd[j]["failed"]) + int(fwd[j]["deferred"])
            m = int(rng.integers(0, 30))
            if m == 0:
                fwd[j]["next"] = int(rng.integers(-2, n))
            elif m == 1:
                fwd[j]["acked"] = fwd[j]["failed"] = fwd[j]["deferred"] = fwd[j]["attempts"] = 0
            elif m == 2:
                fwd[j]["next"] = int(peer[j, int(rng.integers(0, K))])
        if n >= 2:                                                    # node 0's script
            peer[0, 0] = -1 if EMPTY_FROM <= f <= EMPTY_TO else 1
            h, d = (0, 0) if f == 0 else (int(out[-1][1][0, 0]["heard"]), int(out[-1][1][0, 0]["delivered"]))
            if f == RESET_AT:
                h = d = 0
            stats[0, 0]["heard"], stats[0, 0]["delivered"] = h + 2, d + (0 if f in (4, 5) else 1)
            for k in range(1, K):
                if peer[0, k] == 1:
                    peer[0, k] = -1                                   # (slot 0 alone holds node 1)
            a, fl = (0, 0) if f == 0 else (int(out[-1][2][0]["acked"]), int(out[-1][2][0]["failed"]))
            fwd[0]["next"], fwd[0]["acked"], fwd[0]["failed"] = 1, a + 2, fl + 1
        out.append((peer.copy(), stats.copy(), fwd.copy()))
    return out


def play(n, K, p, seq, each=None):
    """the reference over a scene; each(fold index, inputs, ref) after every fold"""
    ref = Ref(n, K, p)
    for f, (peer, stats, fwd) in enumerate(seq):
        ref.fold(peer, stats, fwd)
        if each:
            each(f, (peer, stats, fwd), ref)
    return ref


def conditions(ref):
    """what every scene of two or more nodes shows at least once"""
    t = ref.totals()
    return {"between": ref.log["between_seen"] >= 1, "restart": t["restarted"] >= 1, "cleared": t["cleared"] >= 1,
            "unmatched": t["data_unmatched"] >= 1, "zero_delivered": ref.log["zero_delivered"] >= 1, "partial": ref.log["partial"] >= 1}
