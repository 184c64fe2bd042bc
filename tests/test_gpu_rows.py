"""The row kernels behind every "node list" call of E11, E13, E14 and E15 (rm_rows.hip: k_rows_gather, k_rows_scatter; DESIGN.md
4.21) on the GPU, at every row width in use: 1 word (missed counts), 3 (listening schedules), 4 (traffic schedules), 8 (traffic
counters) and 6 K (watched-link entries, K = 1 and 8).

No expected value comes from the path under test.  A list read is held to the whole-table read (a plain copy) or to a read of the
device table through the rm_*_device pointer; a list update to numpy applying the list in order to a host array, compared with a
read of the device table.  One lone tick of the "lone" scene puts non-zero counters into the tables first.

A full launch is 64 workgroups of 256 lanes, one 64-bit word each: a list of more words than that makes lanes take further words
through the stride loop, which the feature tests' lists of 5000 entries do not for the narrow rows."""
import numpy as np
import pytest

import linkstats_ref as K
import listen_ref as LR
from test_gpu_linkstats import _engine, _ref
from test_gpu_stats import _lone
from util import DeviceArray

pytestmark = pytest.mark.gpu

LANES = 64 * 256
ENTRIES = {1: 17001, 3: 5463}   # (the others: the first count over a full launch, plus two)


def _long_list(n_nodes, words, rng):
    """more words than a full launch has lanes, no multiple of 256 words; holds node 0 and the last node, one node twice in a row,
    and ends on the last node"""
    n = ENTRIES.get(words, LANES // words + 3)
    assert n * words > LANES and (n * words) % 256 != 0
    idx = rng.integers(0, n_nodes, n).astype(np.int32)
    idx[0], idx[1], idx[-1] = 0, n_nodes - 1, n_nodes - 1
    idx[3] = idx[2]
    return idx


def _lists(n_nodes, words, seed):
    rng = np.random.default_rng(seed)
    return [np.array([n_nodes - 1], dtype=np.int32), np.array([0, n_nodes - 1], dtype=np.int32), _long_list(n_nodes, words, rng)]


def _traffic_records(n, rng):
    period = rng.integers(1, 1 << 20, n)
    rows = np.stack([period, rng.integers(0, period), rng.integers(0, period + 1), np.zeros(n, dtype=np.int64)], axis=1).astype(np.int64)
    return np.ascontiguousarray(rows)


def _scene(rsa, k=4, traffic=False):
    """an engine with the counters, the schedules and K watched slots on, after one lone tick -> (eng, nd, DeviceArray to free)"""
    nd, lists, starts, air, sched, _, rows, _, _ = _ref("lone", k)
    eng, d = _engine(rsa, nd, k, rows, stats=True, sched=sched), DeviceArray(lists[0])
    if traffic:
        eng.traffic_set(_traffic_records(nd.n, np.random.default_rng(3)))
    _lone(eng, "sources", d, lists[0], starts[0], air)
    return eng, nd, d


def _apply(cur, idx, recs):
    for j, r in zip(idx, recs):
        cur[j] = r


# ---- 1. and 2. lists of 1 and 2 entries, and a list longer than one full launch, at every width -------------------------------------

def test_width_1_missed_counts(rsa, O):
    eng, nd, d = _scene(rsa)
    try:
        whole = eng.listen_missed()
        assert whole.any()
        np.testing.assert_array_equal(DeviceArray.read(eng.listen_device()[1], np.uint64, nd.n), whole)
        for idx in _lists(nd.n, 1, 11):
            np.testing.assert_array_equal(eng.listen_missed(idx), whole[idx], err_msg="%d entries" % len(idx))
    finally:
        d.free()
        eng.close()


def test_width_3_listening_schedules(rsa, O):
    eng, nd, d = _scene(rsa)
    try:
        p_s, _ = eng.listen_device()
        cur = DeviceArray.read(p_s, rsa.LISTEN_SCHEDULE_DTYPE, nd.n).astype(LR.DTYPE)
        for k, idx in enumerate(_lists(nd.n, 3, 12)):
            recs = LR.schedule(len(idx), 200 + k)[0]
            eng.listen_set(recs, idx)
            _apply(cur, idx, recs)
            np.testing.assert_array_equal(DeviceArray.read(p_s, rsa.LISTEN_SCHEDULE_DTYPE, nd.n), cur, err_msg="%d entries" % len(idx))
    finally:
        d.free()
        eng.close()


def test_width_4_traffic_schedules(rsa, O):
    eng, nd, d = _scene(rsa, traffic=True)
    try:
        rng, p = np.random.default_rng(13), eng.traffic_device()
        cur = DeviceArray.read(p, rsa.TRAFFIC_SCHEDULE_DTYPE, nd.n)
        assert cur["period_us"].all()
        for idx in _lists(nd.n, 4, 13):
            what = "%d entries" % len(idx)
            np.testing.assert_array_equal(eng.traffic_get(idx), cur[idx], err_msg="get, " + what)
            recs = _traffic_records(len(idx), rng).view(rsa.TRAFFIC_SCHEDULE_DTYPE).reshape(-1)
            eng.traffic_set(recs, idx)
            _apply(cur, idx, recs)
            np.testing.assert_array_equal(DeviceArray.read(p, rsa.TRAFFIC_SCHEDULE_DTYPE, nd.n), cur, err_msg="set, " + what)
    finally:
        d.free()
        eng.close()


def test_width_8_traffic_counters(rsa, O):
    eng, nd, d = _scene(rsa)
    try:
        whole, _ = eng.stats_read()
        assert whole["rx_heard"].any() and whole["tx_frames"].any()
        np.testing.assert_array_equal(DeviceArray.read(eng.stats_device()[0], rsa.NODE_STATS_DTYPE, nd.n), whole)
        for idx in _lists(nd.n, 8, 14):
            np.testing.assert_array_equal(eng.stats_read(idx)[0], whole[idx], err_msg="%d entries" % len(idx))
    finally:
        d.free()
        eng.close()


@pytest.mark.parametrize("k", [1, 8])
def test_width_6k_link_entries(rsa, O, k):
    eng, nd, d = _scene(rsa, k)
    try:
        whole, _ = eng.linkstats_read()
        assert whole["heard"].any()
        np.testing.assert_array_equal(DeviceArray.read(eng.linkstats_device()[1], rsa.LINK_STATS_DTYPE, nd.n * k).reshape(nd.n, k), whole)
        for idx in _lists(nd.n, 6 * k, 15):
            np.testing.assert_array_equal(eng.linkstats_read(idx)[0], whole[idx], err_msg="%d entries" % len(idx))
    finally:
        d.free()
        eng.close()


# ---- 3. a list update and, at once, a list read of other nodes: both stage through ONE block ----------------------------------------

SIZES = (1, 300, 1)   # (across the block's first growth and back)


def _pair(n_nodes, size, rng):
    """a: distinct nodes; b: other nodes than a, entry by entry"""
    a = rng.choice(n_nodes, size, replace=False).astype(np.int32)
    b = ((a + 1 + rng.integers(0, n_nodes - 1, size)) % n_nodes).astype(np.int32)
    return a, b


def test_traffic_list_set_followed_at_once_by_a_list_get(rsa, O):
    eng, nd, d = _scene(rsa, traffic=True)
    try:
        rng, p = np.random.default_rng(21), eng.traffic_device()
        cur = DeviceArray.read(p, rsa.TRAFFIC_SCHEDULE_DTYPE, nd.n)
        for k, size in enumerate(SIZES):
            a, b = _pair(nd.n, size, rng)
            recs = _traffic_records(size, rng).view(rsa.TRAFFIC_SCHEDULE_DTYPE).reshape(-1)
            eng.traffic_set(recs, a)
            got = eng.traffic_get(b)
            _apply(cur, a, recs)
            np.testing.assert_array_equal(got, cur[b], err_msg="get %d" % k)
            np.testing.assert_array_equal(DeviceArray.read(p, rsa.TRAFFIC_SCHEDULE_DTYPE, nd.n), cur, err_msg="table after pair %d" % k)
    finally:
        d.free()
        eng.close()


def test_link_list_watch_followed_at_once_by_a_list_read(rsa, O):
    k = 4
    eng, nd, d = _scene(rsa, k)
    try:
        rng = np.random.default_rng(22)
        p_peer, p_tbl, _ = eng.linkstats_device()
        want = K.Table(nd.n, k)
        want.peer[...] = DeviceArray.read(p_peer, np.int32, nd.n * k).reshape(nd.n, k)
        want.t[...] = eng.linkstats_read()[0]
        assert want.t["heard"].any()
        for j, size in enumerate(SIZES):
            a, b = _pair(nd.n, size, rng)
            rows = np.full((size, k), -1, dtype=np.int32)
            rows[:, 0], rows[:, 1] = (a + 1) % nd.n, (a + 2) % nd.n   # (distinct, never the node itself)
            eng.linkstats_watch(rows, a)
            got, _ = eng.linkstats_read(b)
            want.watch(a, rows)
            np.testing.assert_array_equal(got, want.t[b], err_msg="read %d" % j)
            np.testing.assert_array_equal(DeviceArray.read(p_peer, np.int32, nd.n * k).reshape(nd.n, k), want.peer, err_msg="peers after pair %d" % j)
            np.testing.assert_array_equal(DeviceArray.read(p_tbl, rsa.LINK_STATS_DTYPE, nd.n * k).reshape(nd.n, k), want.t,
                                          err_msg="entries after pair %d" % j)
    finally:
        d.free()
        eng.close()


# ---- 4. the totals: with a list, and alone ---------------------------------------------------------------------------------------------

def test_totals_with_a_list_and_alone(rsa, O):
    eng, nd, d = _scene(rsa)
    try:
        idx, none = np.array([nd.n - 1, 0, 5], dtype=np.int32), np.zeros(0, dtype=np.int32)
        for name, read, p_tot in (("counters", eng.stats_read, eng.stats_device()[1]), ("links", eng.linkstats_read, eng.linkstats_device()[2])):
            on_device = DeviceArray.read(p_tot, np.uint64, 2)
            assert on_device.tolist() == [1, 0], name
            want = {"ticks_counted": int(on_device[0]), "ticks_skipped": int(on_device[1])}
            whole, tot = read()
            assert tot == want, name
            part, tot = read(idx)
            assert tot == want, name
            np.testing.assert_array_equal(part, whole[idx], err_msg=name)
            part, tot = read(none)
            assert tot == want and len(part) == 0, name
    finally:
        d.free()
        eng.close()
