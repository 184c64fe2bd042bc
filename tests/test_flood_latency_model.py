"""The host model of tools/flood_latency.py's yardstick (HostFlood: E20 with numpy, for lone ungated ticks over lists that came from
sources()) against the reference state machine of tests/flood_ref.py on random small scenes with made-up tick results: the
yardstick the measurement is compared with computes what the rules say.  No GPU, no oracle."""
import importlib.util
import os

import numpy as np
import pytest

import flood_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("flood_latency", os.path.join(ROOT, "tools", "flood_latency.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _same(h, ref, what):
    tbl = ref.table()
    for f in F.NODE_FIELDS:
        assert [int(v) for v in h.a[f]] == tbl[f], (what, f)
    assert h.totals() == ref.totals(), (what, h.totals(), ref.totals())


@pytest.mark.parametrize("seed, params", [(1, dict(imin_us=2000, doublings=0, max_intervals=3, redundancy=1, max_hops=2, seed=5)),
                                          (2, dict(imin_us=4000, doublings=3, max_intervals=8, redundancy=2, max_hops=255, seed=20)),
                                          (3, dict(imin_us=3, doublings=16, max_intervals=64, redundancy=0, max_hops=255, seed=(1 << 64) - 1)),
                                          (4, dict(imin_us=1 << 32, doublings=1, max_intervals=2, redundancy=255, max_hops=65535, seed=0))])
def test_host_model_against_the_reference(seed, params):
    T = _tool()
    rng = np.random.default_rng(seed)
    n, tick, air, cap = 90, 1000, 640, 40
    h, ref = T.HostFlood(n, **params), F.State(n, **params)
    seeds = [int(v) for v in rng.integers(-2, n + 2, 6)] + [7, 7]
    h.seed_nodes(seeds, 0)
    ref.seed(seeds, 0)
    _same(h, ref, "seeded")
    step = max(tick, params["imin_us"] // 4)
    for k in range(60):
        t = k * step
        lst, count = h.sources(t + 100, cap)
        want, wcount = ref.sources(t + 100, cap)
        assert (lst.tolist(), count) == (want, wcount), k
        # a made-up result: every listed node reaches a few random nodes, most copies delivered; an entry that is not due (a stray)
        # and one outside the table now and then
        lst = lst.copy()
        free = np.flatnonzero(lst < 0)
        if len(free) and k % 3 == 0:
            lst[free[0]] = int(rng.integers(0, n)) if k % 2 else n + 3
            if lst[free[0]] in lst[:free[0]]:
                lst[free[0]] = -1
        off, dst, verdict = [0], [], []
        for j in lst:
            m = int(rng.integers(0, 6)) if j >= 0 else 0
            d = np.sort(rng.choice(n, m, replace=False))
            dst += [int(v) for v in d if v != j]
            off.append(len(dst))
        verdict = np.where(rng.uniform(0, 1, len(dst)) < 0.8, F.DELIVERED, 1).astype(np.uint8)
        rssi = -rng.uniform(40.0, 95.0, len(dst))
        lost = k == 17
        h.advance(lst, np.array(off, dtype=np.uint32), np.array(dst, dtype=np.int32), verdict, rssi, t + 100, air, lost=lost)
        ref.advance(F.records_result(n, lst, t + 100, air, off, dst, verdict, rssi, lost=lost))
        ref.check()
        _same(h, ref, "step %d" % k)
    tot = ref.totals()
    assert tot["covered"] > tot["seeds"] and tot["heard"] > 50 and tot["skipped_slots"] == 1
    if 0 < params["redundancy"] < 255:
        assert tot["suppressed"] > 0
    if params["max_hops"] == 2:
        assert tot["max_hop"] == 2 and tot["covered"] < n


def test_mulhi():
    T = _tool()
    rng = np.random.default_rng(0)
    a = rng.integers(0, 1 << 63, 200, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 200, dtype=np.uint64)
    b = rng.integers(0, 1 << 48, 200, dtype=np.uint64)
    a[:2], b[:2] = np.uint64((1 << 64) - 1), [np.uint64((1 << 64) - 1), np.uint64(0)]
    assert [int(v) for v in T.mulhi(a, b)] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
