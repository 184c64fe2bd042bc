"""The host model of tools/nbtable_latency.py's yardstick (HostNbTable: E22 and E14's pass with numpy) against the reference of
tests/nbtable_ref.py on random small scenes with made-up tick results: the yardstick the measurement is compared with computes what
the rules say.  No GPU, no oracle."""
import importlib.util
import os

import numpy as np
import pytest

import linkstats_ref as LS
import nbtable_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("nbtable_latency", os.path.join(ROOT, "tools", "nbtable_latency.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _same(h, ref, what):
    assert (h.peer == ref.tab.peer).all(), (what, "peer")
    for c in LS.COLS:
        assert (h.s[c] == ref.tab.t[c]).all(), (what, c)
    for f in R.NODE_FIELDS:
        assert h.cnt[f].tolist() == ref.cnt[f], (what, f)
    assert h.totals() == ref.totals(), (what, h.totals(), ref.totals())


@pytest.mark.parametrize("seed, K, params", [(1, 1, dict(timeout_us=3000, min_heard=1, evict_cost=128, require_delivered=1)),
                                             (2, 2, dict(timeout_us=0, min_heard=2, evict_cost=200, require_delivered=0)),
                                             (3, 4, dict(timeout_us=2500, min_heard=0, evict_cost=0, require_delivered=1)),
                                             (4, 8, dict(timeout_us=1 << 62, min_heard=3, evict_cost=(1 << 32) - 1, require_delivered=0)),
                                             (5, 2, dict(timeout_us=1500, min_heard=2, evict_cost=160, require_delivered=0, admit_rssi_dbm=-80.0))])
def test_host_model_against_the_reference(seed, K, params):
    T = _tool()
    rng = np.random.default_rng(seed)
    n, tick = 40, 1000
    h, ref = T.HostNbTable(n, K, **params), R.State(n, K, **params)
    for k in range(50):
        t = k * tick
        # a made-up result: a handful of senders (one twice, one outside the table now and then) each reach a few random nodes,
        # most copies delivered, some with NaN or weak rssi
        src = [int(v) for v in rng.choice(n, 5, replace=False)]
        if k % 4 == 0:
            src.append(src[0])
        if k % 5 == 0:
            src.append(n + 2 if k % 2 else -1)
        off, dst = [0], []
        for j in src:
            m = int(rng.integers(0, 7))
            dst += [int(v) for v in np.sort(rng.choice(n, m, replace=False))]
            off.append(len(dst))
        L = len(dst)
        verdict = np.where(rng.uniform(0, 1, L) < 0.7, R.DELIVERED, 1).astype(np.uint8)
        rssi = rng.choice([-60.0, -60.0, -71.5, -79.0, -90.25, -99.0, np.nan], size=L)
        sinr = rng.uniform(-5.0, 30.0, L) if seed % 2 else None
        pin = None if k % 3 == 0 else rng.integers(-2, n, n).astype(np.int32)
        lost = k == 17
        res = R.Result(np.where((np.array(src) >= 0) & (np.array(src) < n), src, -1), t + 100, off, dst, verdict, rssi, sinr, lost)
        start = np.full(len(src), t + 100, dtype=np.int64)
        if not lost:
            h.count(src, start, np.array(off), np.array(dst, dtype=np.int32), verdict, rssi, sinr)
        ref.count(res)
        _same(h, ref, "count %d" % k)
        h.update(src, start, np.array(off), np.array(dst, dtype=np.int32), verdict, rssi, t + tick, sinr=sinr, pin=pin, lost=lost)
        ref.update(res, t + tick, pin)
        ref.check()
        _same(h, ref, "update %d" % k)
        if k % 7 == 6:
            h.expire(t + tick + 300, pin)
            ref.expire(t + tick + 300, pin)
            _same(h, ref, "expire %d" % k)
    tot = ref.totals()
    assert tot["admitted"] > 20 and tot["skipped_slots"] == 1 and tot["updates"] == 49
    if params["timeout_us"] and params["timeout_us"] < 1 << 40:
        assert tot["evicted_stale"] + tot["expired"] > 0
    if K <= 2:
        assert tot["refused"] > 0 or tot["evicted_poor"] > 0 or tot["evicted_stale"] > 0


def test_q8():
    T = _tool()
    x = np.array([0.0, -0.001953125, -95.0, 12.3456, np.nan, np.inf, -np.inf, 2147483647.9, 2147483648.0, -3e9])
    assert T.q8(x).tolist() == LS.q8(x).tolist()
