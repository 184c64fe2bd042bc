"""Traffic schedules on the device (rm_traffic.hip) against tests/traffic_ref.py, the rule in plain Python
integers.  Every comparison is exact.  Shapes are the smallest at which the kernels can still go wrong: node counts around one
round of 64 lanes and over many units, window counts around 64 and the largest batch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import errmodel_ref as R
import stats_ref as S
import traffic_ref as T
from test_gpu_cca import _bits, _engine as _plain_engine
from test_gpu_cca_batch import _refused
from test_gpu_stats import _launches
from util import DeviceArray, configure_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY, STATE = -1, -4, -5
TICK = 1000
TRAFFIC_KERNELS = ("k_traffic", "k_rows_")   # (name prefixes: the generator's kernels, and what a list update or a list read launches)


def _bare(rsa, n):
    eng = rsa.Engine(0)
    eng.upload_nodes(np.zeros(n), np.arange(n, dtype=np.float64))
    return eng


def _windows(n, first=5000, rng=None):
    """n windows in time order: lengths 1 .. 400, a gap in front of every fifth, every seventh empty"""
    rng = rng or np.random.default_rng(n)
    lo, hi, t = [], [], first
    for b in range(n):
        if b % 5 == 2:
            t += int(rng.integers(1, 300))
        length = 0 if b % 7 == 3 else int(rng.integers(1, 400))
        lo.append(t)
        hi.append(t + length)
        t += length
    return lo, hi


def _mixed(n, lo, hi, seed=1):
    """every kind of record in one table: period 0; a period far above the span with its first packet behind it; a period below a
    window (coalescing); jitter 0, 1 and P; phases that put a due time on a win_lo, a win_hi - 1 and a win_hi.  Tables of more
    than 2000 nodes keep these kinds on every 97th node and on the last ones, and period 0 / far periods elsewhere."""
    rng = np.random.default_rng(seed)
    span = max(hi[-1] - lo[0], 8)
    big = 4 * (hi[-1] + 1)                                   # one packet at most inside the span, at its phase
    edges = [b for b in range(len(lo)) if hi[b] > lo[b]]
    table = []
    for i in range(n):
        kind = i % 10
        if n > 2000 and i % 97 and i < n - 70:
            kind = i % 2
        b = edges[i % len(edges)] if edges else 0
        if kind == 0:
            table.append((0, 0, 0))
        elif kind == 1:
            table.append((1 << 40, (1 << 40) - 1 - i % 1000, i % 3))
        elif kind == 2:
            p = max(1, (hi[b] - lo[b]) // 3)
            table.append((p, int(rng.integers(0, p)), 0))
        elif kind == 3:
            p = int(rng.integers(1, span))
            table.append((p, int(rng.integers(0, p)), 1))
        elif kind in (4, 5):
            p = int(rng.integers(1, 2 * span))
            table.append((p, int(rng.integers(0, p)), p))
        elif kind == 6:
            p = int(rng.integers(2, span))
            table.append((p, int(rng.integers(0, p)), int(rng.integers(0, p + 1))))
        elif kind == 7:
            table.append((big, lo[b], 0))
        elif kind == 8:
            table.append((big, hi[b] - 1, 0))
        else:
            table.append((big, hi[b], 0))
    return table


def _check(eng, table, seed, lo, hi, cap):
    want_rows, want_count, want_tot, _ = T.generate(table, seed, lo, hi, cap)
    rows, count, tot = eng.traffic_generate(seed, lo, hi, cap)
    np.testing.assert_array_equal(count, want_count)
    np.testing.assert_array_equal(rows, want_rows)
    assert tot == want_tot, (tot, want_tot)
    for b in range(len(lo)):                                     # ascending, -1 behind the count
        k = min(int(count[b]), cap)
        assert (np.diff(rows[b, :k]) > 0).all() and (rows[b, k:] == -1).all()
    return want_count, want_tot


# ---- 1. rows, counts and totals over the shapes -----------------------------------------------------------------------------

@pytest.mark.parametrize("n_win", [1, 63, 64, 65, 512])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 70001])
def test_mixed_tables_equal_the_reference(rsa, n, n_win):
    lo, hi = _windows(n_win)
    table = _mixed(n, lo, hi, seed=n + n_win)
    if n == 1:
        table = [(max(1, (hi[-1] - lo[0]) // 7), 0, 3 % max(1, (hi[-1] - lo[0]) // 7))]
    eng = _bare(rsa, n)
    try:
        eng.traffic_set(T.table_rows(table))
        count, tot = _check(eng, table, 0xABCDEF0123456789, lo, hi, max(8, min(n // 2, 300)))
        if n >= 1000:
            assert tot["coalesced"] > 0 and count.max() > 0
            assert (count == 0).any() or n_win == 1
    finally:
        eng.close()


MULTI_ROUND = 2048 * 64 + 1 + 70   # above 2048 rounds of 64 nodes the generator's units own more than one round each


def _chunk(n):
    """nodes per unit, as DESIGN.md 4.19 states the geometry: rounds of 64 nodes, at most 2048 units"""
    rounds = (n + 63) // 64
    return 64 * ((rounds + 2047) // 2048)


def _share_a_unit_across_rounds(row, chunk):
    """does the list hold two sources of one unit that lie in different rounds of it"""
    row = np.asarray(row)
    same_unit = row[1:] // chunk == row[:-1] // chunk
    return bool((same_unit & (row[1:] // 64 != row[:-1] // 64)).any())


@pytest.mark.parametrize("n_win", [65, 512])
def test_units_of_several_rounds(rsa, n_win):
    """a table large enough that a unit walks two rounds: the running positions, the packet sums and the table's tail carry over"""
    n, chunk = MULTI_ROUND, _chunk(MULTI_ROUND)
    assert chunk == 128 and n % chunk not in (0, 64) and (n - 1) // chunk * chunk + 64 < n    # the last unit's second round is partial
    lo, hi = _windows(n_win)
    table = _mixed(n, lo, hi, seed=n_win)
    # every kind of record, densely, across the rounds of the units around node 65 536 (the table's last 70 nodes are dense already)
    dense = _mixed(390, lo, hi, seed=n_win + 1)
    table[65536 - 130:65536 + 260] = dense
    for i in range(0, n - 70, 97):                                       # (three in four of the scattered senders rest: the reference
        if (i // 97) % 4:                                                #  walks every sender through every window)
            table[i] = (0, 0, 0)
    eng = _bare(rsa, n)
    try:
        eng.traffic_set(T.table_rows(table))
        cap, seed = 600, 0x5EED
        want_rows, want_count, want_tot, _ = T.generate(table, seed, lo, hi, cap)
        lists = T.lists_of(want_rows, want_count)
        assert sum(_share_a_unit_across_rounds(l, chunk) for l in lists) >= 10
        assert any(l and l[-1] >= n - 7 for l in lists)                  # a source in the partial last round
        assert want_tot["coalesced"] > 0 and want_tot["truncated"] == 0 and 100 < want_count.max() <= cap
        rows, count, tot = eng.traffic_generate(seed, lo, hi, cap)
        np.testing.assert_array_equal(count, want_count)
        np.testing.assert_array_equal(rows, want_rows)
        assert tot == want_tot
        # clipped at 100: the reference's rows cut there (a row holds the first cap sources), the same counts and packets
        rows, count, tot = eng.traffic_generate(seed, lo, hi, 100)
        np.testing.assert_array_equal(count, want_count)
        np.testing.assert_array_equal(rows, want_rows[:, :100])
        assert tot == dict(want_tot, truncated=int(np.maximum(want_count - 100, 0).sum())) and tot["truncated"] > 0
    finally:
        eng.close()


def test_cap_cuts_inside_a_later_round_of_a_unit(rsa):
    """two whole units send in one window and every third of their nodes in the next: cap ends a row in the second round of the
    first unit, in the second round of the second, and one short of the count"""
    n, chunk = MULTI_ROUND, _chunk(MULTI_ROUND)
    first = 65536 - chunk
    assert chunk == 128 and first % chunk == 0
    table = [(0, 0, 0)] * n
    for i in range(first, first + 2 * chunk):
        table[i] = (1000, 0, 0) if i % 3 else (500, 0, 0)
    table[n - 1] = (1000, 0, 0)                                          # (the last node of the partial round)
    lo, hi = [5000, 5500, 6000], [5001, 5501, 6001]
    want_rows, want_count, _, _ = T.generate(table, 1, lo, hi, 300)
    assert want_count.tolist() == [2 * chunk + 1, sum(1 for i in range(first, first + 2 * chunk) if i % 3 == 0), 2 * chunk + 1]
    eng = _bare(rsa, n)
    try:
        eng.traffic_set(T.table_rows(table))
        for cap in (64 + 36, chunk + 64 + 10, 2 * chunk, 2 * chunk + 1, 300):
            count, tot = _check(eng, table, 1, lo, hi, cap)
            assert tot["truncated"] == int(np.maximum(count - cap, 0).sum())
    finally:
        eng.close()


def test_every_node_in_every_window(rsa):
    n, n_win, length = 5000, 64, 250
    lo = [1000 + b * length for b in range(n_win)]
    hi = [x + length for x in lo]
    table = [(length, i % length, 0) for i in range(n)]
    eng = _bare(rsa, n)
    try:
        eng.traffic_set(T.table_rows(table))
        count, tot = _check(eng, table, 3, lo, hi, n)
        assert (count == n).all() and tot == {"packets": n * n_win, "coalesced": 0, "truncated": 0}
    finally:
        eng.close()


def test_nobody_in_any_window(rsa):
    n = 3000
    lo, hi = _windows(65)
    table = [(0, 0, 0) if i % 2 else (1 << 40, hi[-1] + i, i % 5) for i in range(n)]
    eng = _bare(rsa, n)
    try:
        eng.traffic_set(T.table_rows(table))
        rows, count, tot = eng.traffic_generate(9, lo, hi, 16)
        assert not count.any() and (rows == -1).all() and tot == {"packets": 0, "coalesced": 0, "truncated": 0}
        _check(eng, table, 9, lo, hi, 16)
    finally:
        eng.close()


def test_cap_below_the_largest_count(rsa):
    """the first cap nodes in node order, the true count, truncated as defined -- and nothing outside a row's cap words is written"""
    n, cap = 700, 7
    lo, hi = [0, 100, 100, 400, 1000], [100, 100, 400, 900, 1001]
    table = [(150 + i % 50, i % 100, (i % 3) * 40) for i in range(n)]
    want_rows, want_count, want_tot, _ = T.generate(table, 21, lo, hi, cap)
    assert want_count.max() > 10 * cap and (want_count == 0).any() and ((want_count > 0) & (want_count < cap)).any() and want_tot["truncated"] == int(np.maximum(want_count - cap, 0).sum())
    eng = _bare(rsa, n)
    guard = 64
    d_src = DeviceArray(np.full(guard + len(lo) * cap + guard, -777, dtype=np.int32))
    d_cnt = DeviceArray(np.full(len(lo) + 2, -777, dtype=np.int32))
    d_tot = DeviceArray(np.zeros(3, dtype=np.uint64))
    try:
        eng.traffic_set(T.table_rows(table))
        eng.traffic_generate_device(21, lo, hi, cap, d_src.ptr.value + 4 * guard, d_cnt.ptr.value + 4, d_tot.ptr.value)
        eng.sync()
        got = DeviceArray.read(d_src.ptr.value, np.int32, guard + len(lo) * cap + guard)
        assert (got[:guard] == -777).all() and (got[-guard:] == -777).all()
        np.testing.assert_array_equal(got[guard:-guard].reshape(len(lo), cap), want_rows)
        cnt = DeviceArray.read(d_cnt.ptr.value, np.int32, len(lo) + 2)
        assert cnt[0] == -777 and cnt[-1] == -777
        np.testing.assert_array_equal(cnt[1:-1], want_count)
        tot = DeviceArray.read(d_tot.ptr.value, np.uint64, 3).tolist()
        assert tot == [want_tot["packets"], want_tot["coalesced"], want_tot["truncated"]]
        # cap 1, and a cap above every count
        _check(eng, table, 21, lo, hi, 1)
        _check(eng, table, 21, lo, hi, n + 5)
    finally:
        for d in (d_src, d_cnt, d_tot):
            d.free()
        eng.close()


def test_times_near_the_top_and_the_longest_period(rsa):
    top = 1 << 62
    p40 = 1 << 40
    lo = [top - 3 * p40, top - 2 * p40 + 5, top - p40, top - 1000, top - 1]
    hi = [top - 2 * p40, top - p40, top - 1000, top - 1, top]
    # long windows, long periods (the reference walks packet by packet)
    table = [(p40, 0, 0), (p40, p40 - 1, p40), (p40, 5, 0), (p40, 4, 0), (p40, p40 - 1000, 999), (p40, p40 - 1, 0), (p40, p40 - 2, 1),
             (0, 0, 0), (p40, 123456789, p40 // 2), (p40 // 3, 17, p40 // 3), (p40 // 2 + 1, p40 // 2, 1)] * 7
    # short windows at the very top, short periods
    near_lo, near_hi = [top - 5000, top - 3000, top - 1], [top - 3000, top - 1, top]
    near = [(1, 0, 1), (1, 0, 0), (7, 6, 7), (1000, 999, 1000), (999, 0, 999), (p40, p40 - 1, 0), (p40, p40 - 2, 2), (0, 0, 0), (2500, 1, 2500)] * 8
    eng = _bare(rsa, len(table))
    try:
        eng.traffic_set(T.table_rows(table))
        count, tot = _check(eng, table, T.M64, lo, hi, len(table))
        assert count.min() > 0 and tot["coalesced"] > 0
        eng.upload_nodes(np.zeros(len(near)), np.arange(len(near), dtype=np.float64))
        assert not eng.traffic_enabled()
        eng.traffic_set(T.table_rows(near))
        count, tot = _check(eng, near, 12345, near_lo, near_hi, len(near))
        assert count.min() > 0 and tot["coalesced"] > 10000
        _check(eng, near, 0, [0, top - 5], [3, top], 16)    # a span from 0 to 2^62 with everything between in the gap
    finally:
        eng.close()


# ---- 2. the partition promise ---------------------------------------------------------------------------------------------------

def test_partition_into_calls_and_into_finer_windows(rsa):
    n, n_win, seed, cap = 2000, 64, 77, 2000
    lo, hi = _windows(n_win, first=123456)
    table = _mixed(n, lo, hi, seed=5)
    eng = _bare(rsa, n)
    try:
        eng.traffic_set(T.table_rows(table))
        rows, count, tot = eng.traffic_generate(seed, lo, hi, cap)
        assert tot["packets"] > 10000
        # 64 lone-window calls, and a 20 + 44 split: the same lists
        packets = 0
        for b in range(n_win):
            r1, c1, t1 = eng.traffic_generate(seed, lo[b:b + 1], hi[b:b + 1], cap)
            np.testing.assert_array_equal(r1[0], rows[b], err_msg="window %d alone" % b)
            assert c1[0] == count[b]
            packets += t1["packets"]
        assert packets == tot["packets"]
        ra, ca, ta = eng.traffic_generate(seed, lo[:20], hi[:20], cap)
        rb, cb, tb = eng.traffic_generate(seed, lo[20:], hi[20:], cap)
        np.testing.assert_array_equal(np.concatenate([ra, rb]), rows)
        np.testing.assert_array_equal(np.concatenate([ca, cb]), count)
        assert ta["packets"] + tb["packets"] == tot["packets"] and ta["coalesced"] + tb["coalesced"] == tot["coalesced"]
        # every window cut in three: the same packets, and per coarse window the same nodes
        flo, fhi = [], []
        for a, b in zip(lo, hi):
            c1, c2 = a + (b - a) // 3, a + 2 * (b - a) // 3
            flo += [a, c1, c2]
            fhi += [c1, c2, b]
        rf, cf, tf = eng.traffic_generate(seed, flo, fhi, cap)
        assert tf["packets"] == tot["packets"] and tf["coalesced"] < tot["coalesced"]
        for b in range(n_win):
            union = np.unique(np.concatenate([rf[3 * b + j, :cf[3 * b + j]] for j in range(3)]))
            np.testing.assert_array_equal(union, rows[b, :count[b]], err_msg="window %d" % b)
    finally:
        eng.close()


# ---- 3. list updates and the node table's lifetime ----------------------------------------------------------------------------------

def test_list_updates_and_lifetime(rsa):
    n = 1500
    nd, _ = R.nodes(n)
    eng = _plain_engine(rsa, nd, R.PARAMS)
    lo, hi = [0, 700], [700, 2000]
    try:
        for call in (eng.traffic_get, eng.traffic_device, lambda: eng.traffic_generate(1, lo, hi, 8)):   # before the first set
            _refused(rsa, eng, STATE, call)
        assert not eng.traffic_enabled()
        rng = np.random.default_rng(4)
        cur = np.zeros((n, 4), dtype=np.int64)
        cur[:, 0] = rng.integers(1, 5000, n)
        cur[:, 1] = rng.integers(0, cur[:, 0])
        cur[:, 2] = rng.integers(0, cur[:, 0] + 1)
        cur[::9] = 0
        eng.traffic_set(cur)
        assert eng.traffic_enabled()
        np.testing.assert_array_equal(eng.traffic_get().view(np.int64).reshape(n, 4), cur)
        _check(eng, cur[:, :3].tolist(), 5, lo, hi, n)
        # a list changes only the listed nodes; of a node named twice the last entry wins
        idx = np.array([7, 0, 7, n - 1, 64], dtype=np.int32)
        recs = np.array([(1500, 0, 3, 0), (2000, 1999, 2000, 0), (3000, 2999, 0, 0), (0, 0, 0, 0), (1, 0, 1, 0)], dtype=np.int64)
        eng.traffic_set(recs, idx)
        for j, r in zip(idx, recs):
            cur[j] = r
        assert cur[7].tolist() == [3000, 2999, 0, 0]
        np.testing.assert_array_equal(eng.traffic_get().view(np.int64).reshape(n, 4), cur)
        np.testing.assert_array_equal(eng.traffic_get(idx).view(np.int64).reshape(-1, 4), cur[idx])
        np.testing.assert_array_equal(DeviceArray.read(eng.traffic_device(), np.int64, 4 * n).reshape(n, 4), cur)
        # a long list with many duplicates, followed at once by a list read
        big = rng.integers(0, n, 5000).astype(np.int32)
        recs = np.zeros((5000, 4), dtype=np.int64)
        recs[:, 0] = rng.integers(1, 900, 5000)
        recs[:, 1] = rng.integers(0, recs[:, 0])
        recs[:, 2] = recs[:, 0] * (rng.integers(0, 2, 5000))
        eng.traffic_set(recs, big)
        for j, r in zip(big, recs):
            cur[j] = r
        np.testing.assert_array_equal(eng.traffic_get(big).view(np.int64).reshape(-1, 4), cur[big])
        np.testing.assert_array_equal(eng.traffic_get().view(np.int64).reshape(n, 4), cur)
        _check(eng, cur[:, :3].tolist(), 6, lo, hi, 64)
        # an invalid entry anywhere changes nothing
        for pos in (0, 2, 4):
            bad = np.array([(10, 0, 0, 0)] * 5, dtype=np.int64)
            bad[pos] = (10, 10, 0, 0)
            _refused(rsa, eng, INVALID, lambda: eng.traffic_set(bad, idx))
        _refused(rsa, eng, INVALID, lambda: eng.traffic_set(recs[:3], np.array([1, n, 2], dtype=np.int32)))
        whole = cur.copy()
        whole[n - 1] = (5, 0, 6, 0)
        _refused(rsa, eng, INVALID, lambda: eng.traffic_set(whole))
        np.testing.assert_array_equal(eng.traffic_get().view(np.int64).reshape(n, 4), cur)
        # the medium and the nodes may change: the table stays
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
        eng.seed(3)
        eng.update_node(5, float(nd.x[5]) + 1.0, float(nd.y[5]), float(nd.z[5]), float(nd.txpower[5]), int(nd.channel[5]), 1, 1.0, 1.0)
        eng.upload_table(nd)
        assert eng.traffic_enabled()
        np.testing.assert_array_equal(eng.traffic_get().view(np.int64).reshape(n, 4), cur)
        # another node count clears the feature
        half, _ = R.nodes(n // 2)
        eng.upload_table(half)
        assert not eng.traffic_enabled()
        _refused(rsa, eng, STATE, eng.traffic_get)
        _refused(rsa, eng, STATE, lambda: eng.traffic_generate(1, lo, hi, 8))
        eng.traffic_set(np.zeros((n // 2, 4), dtype=np.int64))
        assert eng.traffic_enabled() and not eng.traffic_get().view(np.int64).any()
        # clear: RM_ERR_STATE afterwards; a new set starts from an empty table
        eng.traffic_set(np.array([(10, 0, 0, 0)], dtype=np.int64), np.array([3], dtype=np.int32))
        eng.traffic_clear()
        assert not eng.traffic_enabled()
        for call in (eng.traffic_get, eng.traffic_device, lambda: eng.traffic_generate(1, lo, hi, 8)):
            _refused(rsa, eng, STATE, call)
        eng.traffic_clear()                                          # (clearing twice is fine)
        eng.traffic_set(np.array([(20, 1, 0, 0)], dtype=np.int64), np.array([4], dtype=np.int32))
        got = eng.traffic_get().view(np.int64).reshape(-1, 4)
        assert got[4].tolist() == [20, 1, 0, 0] and not got[:4].any() and not got[5:].any()
    finally:
        eng.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    n = 100
    eng = _bare(rsa, n)
    d_src, d_cnt = DeviceArray(np.full(1024, -5, dtype=np.int32)), DeviceArray(np.full(16, -5, dtype=np.int32))
    try:
        tbl = np.zeros((n, 4), dtype=np.int64)
        tbl[:, 0] = 50
        # before the first set
        lo1, hi1 = np.array([0], dtype=np.int64), np.array([10], dtype=np.int64)
        assert L.rm_traffic_generate_device(eng._h, 1, 1, lo1.ctypes.data, hi1.ctypes.data, 4, d_src.ptr.value, d_cnt.ptr.value, None) == STATE
        eng.traffic_set(tbl)
        top = 1 << 62
        bad_windows = {
            "a negative win_lo": ([-1, 5], [3, 9]),
            "win_lo above win_hi": ([0, 9], [3, 8]),
            "win_hi above 2^62": ([0, 5], [3, top + 1]),
            "overlapping": ([0, 2], [3, 9]),
            "out of time order": ([10, 0], [20, 5]),
        }
        for what, (lo, hi) in bad_windows.items():
            assert not T.valid_windows(lo, hi), what
            _refused(rsa, eng, INVALID, lambda: eng.traffic_generate(1, lo, hi, 4))
            _refused(rsa, eng, INVALID, lambda: eng.traffic_generate_device(1, lo, hi, 4, d_src.ptr.value, d_cnt.ptr.value))
        _refused(rsa, eng, INVALID, lambda: eng.traffic_generate(1, [], [], 4))                                      # n_ticks 0
        _refused(rsa, eng, INVALID, lambda: eng.traffic_generate(1, list(range(513)), list(range(513)), 1))          # above RM_MAX_BATCH
        _refused(rsa, eng, INVALID, lambda: eng.traffic_generate_device(1, [0], [10], 0, d_src.ptr.value, d_cnt.ptr.value))
        _refused(rsa, eng, INVALID, lambda: eng.traffic_generate_device(1, [0], [10], -3, d_src.ptr.value, d_cnt.ptr.value))
        _refused(rsa, eng, CAPACITY, lambda: eng.traffic_generate_device(1, [0, 10], [10, 20], (1 << 26) + 1, d_src.ptr.value, d_cnt.ptr.value))
        _refused(rsa, eng, CAPACITY, lambda: eng.traffic_generate_device(1, list(range(512)), list(range(512)), (1 << 18) + 1, d_src.ptr.value,
                                                                          d_cnt.ptr.value))
        # NULLs, a negative count
        for args in ((None, hi1.ctypes.data, 4, d_src.ptr.value, d_cnt.ptr.value), (lo1.ctypes.data, None, 4, d_src.ptr.value, d_cnt.ptr.value),
                     (lo1.ctypes.data, hi1.ctypes.data, 4, None, d_cnt.ptr.value), (lo1.ctypes.data, hi1.ctypes.data, 4, d_src.ptr.value, None)):
            assert L.rm_traffic_generate_device(eng._h, 1, 1, *args, None) == INVALID
        assert L.rm_traffic_generate_device(None, 1, 1, lo1.ctypes.data, hi1.ctypes.data, 4, d_src.ptr.value, d_cnt.ptr.value, None) == INVALID
        host = np.zeros(8, dtype=np.int32)
        assert L.rm_traffic_generate(eng._h, 1, 1, lo1.ctypes.data, hi1.ctypes.data, 4, None, host.ctypes.data, None) == INVALID
        assert L.rm_traffic_generate(eng._h, 1, 1, lo1.ctypes.data, hi1.ctypes.data, 4, host.ctypes.data, None, None) == INVALID
        idx = np.array([1, 2], dtype=np.int32)
        assert L.rm_traffic_set(eng._h, idx.ctypes.data, 2, None) == INVALID and L.rm_traffic_set(eng._h, idx.ctypes.data, -1, tbl.ctypes.data) == INVALID
        assert L.rm_traffic_set(None, idx.ctypes.data, 2, tbl.ctypes.data) == INVALID
        assert L.rm_traffic_set(eng._h, None, n - 1, tbl.ctypes.data) == INVALID                 # without a list n is the node count
        assert L.rm_traffic_get(eng._h, idx.ctypes.data, 2, None) == INVALID and L.rm_traffic_get(eng._h, None, n + 1, tbl.ctypes.data) == INVALID
        assert L.rm_traffic_get(None, None, 0, None) == INVALID and L.rm_traffic_clear(None) == INVALID and L.rm_traffic_device(None, None) == INVALID
        assert L.rm_traffic_device(eng._h, None) == INVALID and eng.traffic_device()
        assert L.rm_traffic_enabled(None) == 0
        _refused(rsa, eng, INVALID, lambda: eng.traffic_get(np.array([0, n], dtype=np.int32)))
        # nothing of all this was written or changed
        eng.sync()
        assert (DeviceArray.read(d_src.ptr.value, np.int32, 1024) == -5).all() and (DeviceArray.read(d_cnt.ptr.value, np.int32, 16) == -5).all()
        np.testing.assert_array_equal(eng.traffic_get().view(np.int64).reshape(n, 4), tbl)
        # the largest n_ticks * cap is taken (2^27 words would be 512 MiB: the test stays at a shape the rule names, 512 x 2^10)
        lo, hi = list(range(0, 5120, 10)), list(range(10, 5130, 10))
        rows, count, tot = eng.traffic_generate(1, lo, hi, 1 << 10)
        assert rows.shape == (512, 1024) and int(count.sum()) == tot["packets"] - tot["coalesced"] > 0
    finally:
        d_src.free()
        d_cnt.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import radio_sim_amd as rsa
eng = rsa.Engine(0)
try:
    eng.upload_nodes(np.zeros(4), np.arange(4.0))
    try:
        eng.traffic_set(np.zeros((4, 4), dtype=np.int64))
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        assert not eng.traffic_enabled()
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_set_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)


# ---- 5. end to end: the generated rows as source lists ----------------------------------------------------------------------------------

def _same(a, b, what, pkt=True):
    assert a.count == b.count, (what, a.count, b.count)
    for f in ("dst", "verdict") + (("pkt",) if pkt else ()):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg="%s: %s" % (what, f))
    np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr), err_msg=what + ": sinr")


@pytest.mark.parametrize("medium", ["sinr", "udgm"])
def test_generated_rows_feed_the_batches(rsa, O, medium):
    if medium == "sinr":
        nd, _ = R.nodes(1500, seed=5)

        def make():
            return _plain_engine(rsa, nd, R.PARAMS, 1 << 20)
    else:
        nd = S.scene_udgm()[0]

        def make():
            e = rsa.Engine(0)
            configure_engine(e, nd, "udgm", {})
            e.set_link_capacity(1 << 20)
            return e
    n_ticks, cap, seed, air = 6, 96, 2024, 640
    period = 40 * TICK
    tb = [2 * period + b * TICK for b in range(n_ticks)]        # (every node is in its steady state after one period)
    te = [t + TICK for t in tb]
    starts = [t + 100 for t in tb]
    table = [(0, 0, 0) if i % 11 == 0 else (period, (i * 7919) % period, period) for i in range(nd.n)]
    want_rows, want_count, _, _ = T.generate(table, seed, tb, te, cap)
    lists = T.lists_of(want_rows, want_count)
    assert 10 < want_count.min() and want_count.max() < cap
    engs = [make() for _ in range(3)]
    gen, host, padded = engs
    d_src, d_cnt = DeviceArray(nbytes=4 * n_ticks * cap), DeviceArray(nbytes=4 * n_ticks)
    dev = [DeviceArray(np.array(l, dtype=np.int32)) for l in lists]
    try:
        for e in (gen, padded):
            e.traffic_set(T.table_rows(table))
        rows_at = [d_src.ptr.value + 4 * b * cap for b in range(n_ticks)]
        # the rows as they lie in device memory, n_src = count
        gen.traffic_generate_device(seed, tb, te, cap, d_src.ptr.value, d_cnt.ptr.value)
        gen.sync()
        count = DeviceArray.read(d_cnt.ptr.value, np.int32, n_ticks)
        np.testing.assert_array_equal(count, want_count)
        gen.batch_run_sources_device(tb, te, rows_at, count.tolist(), starts, [air] * n_ticks)
        host.batch_run_sources_device(tb, te, [d.ptr.value for d in dev], [len(l) for l in lists], starts, [air] * n_ticks)
        links = 0
        for b in range(n_ticks):
            g, h = gen.batch_result_copy(b, int(count[b]), cap=1 << 20), host.batch_result_copy(b, len(lists[b]), cap=1 << 20)
            _same(g, h, "%s tick %d" % (medium, b))
            links += h.count
        assert links > 500
        # the padded form: n_src = cap, count never read back -- the same links with the same packet numbers
        padded.traffic_generate_device(seed, tb, te, cap, d_src.ptr.value, d_cnt.ptr.value)
        padded.batch_run_sources_device(tb, te, rows_at, [cap] * n_ticks, starts, [air] * n_ticks)
        for b in range(n_ticks):
            _same(padded.batch_result_copy(b, cap, cap=1 << 20), host.batch_result_copy(b, len(lists[b]), cap=1 << 20), "%s padded tick %d" % (medium, b))
        if medium == "sinr":
            # through the CSMA-CA gated batch, frames that outlive their ticks: the generated rows against the host's lists
            far = [t + 100 * TICK for t in tb]
            rest = ([t + 100 for t in far], [8128] * n_ticks, [t + 50 for t in far], -90.0, rsa.Engine.csma_params(4, 3, 5, 9, None))
            n_gen = gen.batch_run_sources_csma_device(far, [t + TICK for t in far], rows_at, count.tolist(), *rest)
            n_host = host.batch_run_sources_csma_device(far, [t + TICK for t in far], [d.ptr.value for d in dev], [len(l) for l in lists], *rest)
            np.testing.assert_array_equal(n_gen, n_host)
            assert int(np.sum(n_host)) > 0
            for b in range(n_ticks):
                if int(n_host[b]):
                    _same(gen.batch_result_copy(b, int(n_gen[b]), cap=1 << 20), host.batch_result_copy(b, int(n_host[b]), cap=1 << 20),
                          "csma tick %d" % b)
    finally:
        for d in dev + [d_src, d_cnt]:
            d.free()
        for e in engs:
            e.close()


def test_no_schedule_no_launch_and_the_evaluating_calls_launch_what_they_did(rsa, O):
    """an evaluating call's kernel-launch record does not know the feature: the same kernels, the same number of times, on a context
    that never set a schedule, on one that has set and generated, and after a clear; and no k_traffic* without a generate"""
    nd, lists, starts, air = R.scene_batch(False)
    lists = [l for l in lists if len(l)]
    starts = starts[:len(lists)]
    dev = [DeviceArray(l) for l in lists]

    def record(prepare):
        eng = _plain_engine(rsa, nd, R.PARAMS, 1 << 20)
        try:
            seen = prepare(eng)
            eng.profile_enable(1)
            eng.batch_run_sources_device(starts, [s + TICK for s in starts], [d.ptr.value for d in dev], [len(l) for l in lists], starts,
                                         [air] * len(lists))
            eng.sync()
            n, order = _launches(eng)
            return n, order, seen
        finally:
            eng.close()

    def generated(eng):
        eng.profile_enable(1)
        eng.traffic_set(np.array([(100, i % 100, 100, 0) for i in range(nd.n)], dtype=np.int64))
        rows, count, tot = eng.traffic_generate(1, [0, 50], [50, 200], 64)
        assert tot["packets"] > 0
        n, _ = _launches(eng)
        eng.profile_enable(0)
        return n

    def cleared(eng):
        generated(eng)
        eng.traffic_clear()

    try:
        plain, order, _ = record(lambda eng: None)
        assert plain and not [k for k in plain if k.startswith(TRAFFIC_KERNELS)], order
        on, order_on, seen = record(generated)
        assert {k: v for k, v in seen.items() if k.startswith(TRAFFIC_KERNELS)} == {"k_traffic_count": 1, "k_traffic_scan": 1, "k_traffic_write": 1}
        assert on == plain and order_on == order, (on, plain)
        off, order_off, _ = record(cleared)
        assert off == plain and order_off == order
    finally:
        for d in dev:
            d.free()
