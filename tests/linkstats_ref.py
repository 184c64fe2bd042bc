"""Reference of the watched-link statistics, on top of the untouched oracle: q8 in numpy float64 straight
from the rule, a Table with the watch rule (keep / clear) and the per-link additions over the oracle's per-tick results, and the
rule every scene's watch rows come from (rows_first_heard), derived from the reference's results alone.  No engine code is involved
and the library's exports are never the source of an expected value.  tests/test_linkstats_ref.py holds the scenes' conditions for
this reference alone, so that no GPU test passes vacuously."""
import numpy as np

from oracle import oracle as O

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
COLS = ("heard", "delivered", "rssi_q8_sum", "sinr_q8_sum", "first_start_us", "last_start_us")
DTYPE = np.dtype([("heard", "<u8"), ("delivered", "<u8"), ("rssi_q8_sum", "<i8"), ("sinr_q8_sum", "<i8"),
                  ("first_start_us", "<i8"), ("last_start_us", "<i8")])
CLEARED = (0, 0, 0, 0, I64_MAX, I64_MIN)
KS = (1, 2, 4, 8)


def q8(x):
    """the rule: 0 unless fabs(x) < 2147483648.0 (NaN and the infinities: 0), otherwise floor(x * 256.0 + 0.5) -- one rounding per
    operation in float64 -- as int64"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.fabs(x) < 2147483648.0
        v = np.floor(np.where(ok, x, 0.0) * 256.0 + 0.5)
    return np.where(ok, v, 0.0).astype(np.int64)


def valid(n_nodes, K, rows, nodes=None):
    """what rm_linkstats_watch accepts: rows [n][K]"""
    if K not in KS:
        return False
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, K)
    if nodes is None:
        if len(rows) != n_nodes:
            return False
        nodes = np.arange(n_nodes)
    nodes = [int(j) for j in np.asarray(nodes).reshape(-1)]
    if len(nodes) != len(rows) or len(set(nodes)) != len(nodes):
        return False
    for j, row in zip(nodes, rows.tolist()):
        if not 0 <= j < n_nodes:
            return False
        seen = [p for p in row if p != -1]
        if any(not 0 <= p < n_nodes or p == j for p in seen) or len(set(seen)) != len(seen):
            return False
    return True


class Table:
    """the tables after a sequence of watch calls and evaluated ticks, and the totals"""

    def __init__(self, n, K):
        assert K in KS
        self.n, self.K = n, K
        self.peer = np.full((n, K), -1, dtype=np.int32)
        self.t = np.zeros((n, K), dtype=DTYPE)
        self.t[...] = CLEARED
        self.counted = self.skipped = 0

    def watch(self, nodes, rows):
        """rows [len(nodes)][K] for the listed nodes (None: all): a slot whose peer stays keeps its entry, one whose peer changes
        is cleared"""
        rows = np.asarray(rows, dtype=np.int32).reshape(-1, self.K)
        assert valid(self.n, self.K, rows, nodes)
        nodes = np.arange(self.n) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
        changed = self.peer[nodes] != rows
        self.peer[nodes] = rows
        jj, kk = np.nonzero(changed)
        self.t[nodes[jj], kk] = CLEARED

    def add(self, new_packets, res, verdict=None, sinr=True):
        """one evaluated tick: the oracle's TickResult `res` over new_packets (res.pkt counts their positions; src outside
        0 .. n-1: padding); verdict: another final verdict column; sinr: the medium has the sinr column
        -> (matched links, unmatched links)"""
        new = np.atleast_1d(new_packets)
        if len(new) == 0:
            return 0, 0  # an empty tick changes nothing
        self.counted += 1
        pkt, dst = np.asarray(res.pkt, dtype=np.int64), np.asarray(res.dst, dtype=np.int64)
        if len(pkt) == 0:
            return 0, 0
        v = np.asarray(res.verdict if verdict is None else verdict)
        src = new["src"][pkt].astype(np.int64)
        start = new["start_us"][pkt].astype(np.int64)
        ok = (src >= 0) & (src < self.n) & (dst >= 0) & (dst < self.n)
        hit = (self.peer[np.where(ok, dst, 0)] == src[:, None]) & ok[:, None]
        m = hit.any(axis=1)
        j, k = dst[m], hit[m].argmax(axis=1)
        one = np.uint64(1)
        np.add.at(self.t["heard"], (j, k), one)
        np.add.at(self.t["delivered"], (j, k), (v[m] == O.DELIVERED).astype(np.uint64))
        np.add.at(self.t["rssi_q8_sum"], (j, k), q8(np.asarray(res.rssi)[m]))
        if sinr:
            np.add.at(self.t["sinr_q8_sum"], (j, k), q8(np.asarray(res.sinr)[m]))
        np.minimum.at(self.t["first_start_us"], (j, k), start[m])
        np.maximum.at(self.t["last_start_us"], (j, k), start[m])
        return int(m.sum()), int((~m).sum())

    def skip(self):
        self.skipped += 1

    def reset(self):
        """rm_linkstats_reset: the entries and the totals, not the peers"""
        self.t[...] = CLEARED
        self.counted = self.skipped = 0

    def totals(self):
        return {"ticks_counted": self.counted, "ticks_skipped": self.skipped}


def equal(got, want, what=""):
    """exact equality of whole entry tables (got: the engine's structured array [n][K])"""
    assert got.dtype.names == COLS, got.dtype
    assert got.shape == want.t.shape, (what, got.shape, want.t.shape)
    for c in COLS:
        np.testing.assert_array_equal(got[c], want.t[c], err_msg="%s: column %s" % (what, c))


def rows_first_heard(n, K, runs):
    """the watch rule of every scene: runs = [(new_packets, TickResult)] in tick order, walked in (tick, link) order; node j's
    r-th distinct heard source goes to slot (j + r) % K for r < K, later sources are not watched -> int32 [n][K]"""
    rows = np.full((n, K), -1, dtype=np.int32)
    seen = [[] for _ in range(n)]
    for new, res in runs:
        new = np.atleast_1d(new)
        for q, j in zip(np.asarray(res.pkt).tolist(), np.asarray(res.dst).tolist()):
            s = int(new["src"][q])
            if not (0 <= s < n and 0 <= j < n) or s == j:
                continue
            have = seen[j]
            if len(have) < K and s not in have:
                rows[j, (j + len(have)) % K] = s
                have.append(s)
    return rows


def table_of(n, K, rows, runs, verdicts=None, sinr=True):
    """the reference after watching `rows` and running `runs` -> (Table, matched, unmatched)"""
    t = Table(n, K)
    t.watch(None, rows)
    matched = unmatched = 0
    for i, (new, res) in enumerate(runs):
        a, b = t.add(new, res, None if verdicts is None else verdicts[i], sinr)
        matched, unmatched = matched + a, unmatched + b
    return t, matched, unmatched


def conditions(t, matched, unmatched):
    """what a scene has to show"""
    h, d = t.t["heard"], t.t["delivered"]
    return {"matched": matched, "unmatched": unmatched, "heard2": int((h >= 2).sum()), "partly": int(((d > 0) & (d < h)).sum()),
            "slots_hit": [int((h[:, k] > 0).sum()) for k in range(t.K)]}
