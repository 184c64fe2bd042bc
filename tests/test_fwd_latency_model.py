"""The host model of tools/fwd_latency.py's yardstick (HostQueues: E19 with numpy, for lists without duplicates) against the
reference state machine of tests/fwd_ref.py on random small scenes with made-up tick results: the yardstick the measurement is
compared with computes what the rules say.  No GPU, no oracle."""
import importlib.util
import os

import numpy as np
import pytest

import fwd_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("fwd_latency", os.path.join(ROOT, "tools", "fwd_latency.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _same(h, ref, what):
    tbl = ref.table()
    for f in h.c:
        assert h.c[f].tolist() == tbl[f], (what, f)
    assert h.ready.tolist() == tbl["ready_us"] and h.next.tolist() == tbl["next"] and h.tries.tolist() == tbl["tries"], what
    assert h.queue_max.tolist() == tbl["queue_max"] and h.t == ref.totals(), (what, h.t, ref.totals())
    (o, hp, b, e), length = h.queues()
    got = [[(int(o[j, s]), int(hp[j, s]), int(b[j, s]), int(e[j, s])) for s in range(int(length[j]))] for j in range(ref.n)]
    assert got == ref.queues(), what


@pytest.mark.parametrize("seed, params", [(1, dict(queue_slots=2, max_retries=1, min_be=0, max_be=2, max_hops=3, backoff_unit_us=1000, seed=5)),
                                          (2, dict(queue_slots=8, max_retries=3, min_be=3, max_be=5, max_hops=64, backoff_unit_us=1000, seed=19)),
                                          (3, dict(queue_slots=1, max_retries=0, min_be=0, max_be=0, max_hops=255, backoff_unit_us=0, seed=0))])
def test_host_model_against_the_reference(seed, params):
    T = _tool()
    rng = np.random.default_rng(seed)
    n, tick, air = 90, 1000, 640
    parent = np.array([-1] + [int(rng.integers(0, j)) for j in range(1, n)], dtype=np.int32)
    parent[n - 1] = n - 1           # (itself: no route)
    parent[n - 2] = n + 3           # (outside the table: no route)
    h, ref = T.HostQueues(n, **params), F.State(n, **params)
    h.set_next(parent, [0])
    ref.set_next(parent, [0], 0)
    seen = {"rejected": 0, "ttl": 0, "retries": 0, "full": 0}
    for k in range(60):
        t = k * tick
        if k % 3 == 0:
            src = rng.choice(n, 40, replace=False)
            h.inject(src, t)
            ref.inject(src, t)
            _same(h, ref, "inject %d" % k)
        cap = 50 if k % 2 else n
        lst, count = h.sources(t + 100, cap)
        want, wcount = ref.sources(t + 100, cap)
        assert (lst.tolist(), count) == (want, wcount)
        delivered = rng.random(cap) < 0.7
        off, dst = [0], []
        for p, j in enumerate(lst.tolist()):
            if j >= 0 and delivered[p]:
                dst.append(int(h.next[j]))
            off.append(len(dst))
        h.advance(lst, delivered, t + 100, air)
        ref.advance(F.records_result(n, lst, t + 100, air, off, dst, [F.DELIVERED] * len(dst)))
        ref.check()
        _same(h, ref, "step %d" % k)
    tot = ref.totals()
    assert tot["arrived"] > 0 and tot["dropped_no_route"] > 0
    if params["queue_slots"] == 2:
        assert sum(ref.c["rejected"]) > 0 and tot["dropped_ttl"] > 0 and tot["dropped_retries"] > 0 and tot["dropped_full"] > 0
