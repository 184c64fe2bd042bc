"""Traffic schedules without a device: 1. the REFERENCE (tests/traffic_ref.py) against answers worked out
by hand, and the partition promise on it; 2. the library's pure host functions rm_traffic_due and rm_traffic_validate against that
reference; 3. the same functions in a stand-alone program under the host sanitizers (tests/cpp/traffic_host_san_test.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import traffic_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1


# ---- 1. the reference alone --------------------------------------------------------------------------------------------------

def test_mix64_known_answers():
    # splitmix64's finaliser: the first outputs of the generator seeded with 0 are mix64 of the multiples of the increment
    assert T.mix64(0) == 0
    assert T.mix64(T.GOLDEN) == 0xE220A8397B1DCDAF
    assert T.mix64((2 * T.GOLDEN) & T.M64) == 0x6E789E6AA1B965F4
    assert T.mix64((3 * T.GOLDEN) & T.M64) == 0x06C45D188009454F


def test_no_jitter_by_hand():
    s = (100, 30, 0)
    assert [T.due(s, 7, 3, k) for k in range(4)] == [30, 130, 230, 330]
    # the edges: due == win_lo is in, due == win_hi is out
    table = [s]
    rows, count, totals, packets = T.generate(table, 7, [0, 30, 31, 130, 131], [30, 31, 130, 131, 231], 2)
    assert count.tolist() == [0, 1, 0, 1, 1] and rows[:, 0].tolist() == [-1, 0, -1, 0, 0] and (rows[:, 1] == -1).all()
    assert totals == {"packets": 3, "coalesced": 0, "truncated": 0} and packets == {(0, 0), (0, 1), (0, 2)}
    # coalescing: five packets in one window are one source
    rows, count, totals, _ = T.generate(table, 7, [0], [500], 1)
    assert count.tolist() == [1] and totals == {"packets": 5, "coalesced": 4, "truncated": 0}
    # three nodes, cap 2: the first two in node order, the true count, truncated 1; period 0 never sends
    rows, count, totals, _ = T.generate([(10, 0, 0), (0, 0, 0), (10, 5, 0), (10, 9, 0)], 1, [0, 10], [10, 11], 2)
    assert rows.tolist() == [[0, 2], [0, -1]] and count.tolist() == [3, 1] and totals == {"packets": 4, "coalesced": 0, "truncated": 1}


def test_jitter_is_the_high_half_of_the_product():
    seed, node = 0x1234, 5
    for k in range(50):
        h = T.mix64(T.mix64(T.mix64(seed + T.GOLDEN) ^ node) ^ k)
        for jitter in (1, 2, 1000, 1 << 40):
            j = T.jitter_of((1 << 40, 0, jitter), seed, node, k)
            assert j == (h * jitter) >> 64 and 0 <= j < jitter
    assert T.jitter_of((1000, 0, 1), seed, node, 3) == 0     # jitter 1 is no jitter at all
    # jitter = period: once per period, due strictly increasing
    s = (1000, 0, 1000)
    d = [T.due(s, seed, node, k) for k in range(200)]
    assert all(k * 1000 <= d[k] < (k + 1) * 1000 for k in range(200)) and len(set(x % 1000 for x in d)) > 150
    # the node index enters as an unsigned 32-bit word, the packet number as a 64-bit one
    assert T.jitter_of(s, seed, 1, 0) != T.jitter_of(s, seed, 2, 0) and T.jitter_of(s, seed, 1, 1 << 32) != T.jitter_of(s, seed, 1, 0)


def _mixed_table(rng, n, span):
    table = []
    for i in range(n):
        kind = i % 6
        if kind == 0:
            table.append((0, 0, 0))
        elif kind == 1:
            table.append((span * 50, int(rng.integers(0, span * 50)), 0))
        else:
            p = int(rng.integers(1, span))
            table.append((p, int(rng.integers(0, p)), (0, 1, p, int(rng.integers(0, p + 1)))[kind - 2]))
    return table


def test_partition_promise_on_the_reference():
    rng = np.random.default_rng(15)
    table = _mixed_table(rng, 60, 4000)
    a, b = 1000, 9000
    _, _, tot, want = T.generate(table, 99, [a], [b], 64)
    assert tot["packets"] == len(want) > 100
    for trial in range(5):
        cuts = sorted(set(rng.integers(a, b, 12).tolist()) | {a, b})
        lo, hi = cuts[:-1], cuts[1:]
        _, _, tot2, got = T.generate(table, 99, lo, hi, 64)
        assert got == want and tot2["packets"] == tot["packets"]
        # ... and into calls
        h = len(lo) // 2
        _, _, _, g1 = T.generate(table, 99, lo[:h], hi[:h], 64)
        _, _, _, g2 = T.generate(table, 99, lo[h:], hi[h:], 64)
        assert g1 | g2 == want and not (g1 & g2)


# ---- 2. the library's pure host functions against the reference ------------------------------------------------------------------

def _due(L, s, seed, node, k):
    from radio_sim_amd import _lib
    rec = _lib.TrafficSchedule(*(list(s) + [0] * (4 - len(s))))
    out = C.c_int64(-12345)
    rc = L.rm_traffic_due(C.byref(rec), seed, node, k, C.byref(out))
    return rc, out.value


def test_rm_traffic_due_equals_the_reference(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(151)
    scheds = [(100, 30, 0), (100, 30, 1), (100, 99, 100), (1, 0, 0), (1, 0, 1), (1 << 40, (1 << 40) - 1, 1 << 40), (1 << 40, 0, 0),
              (1 << 22, 12345, 1 << 22), (1 << 21, 7, 999), (125000, 124999, 62500)]
    for _ in range(20):
        p = int(rng.integers(1, 1 << 40))
        scheds.append((p, int(rng.integers(0, p)), int(rng.integers(0, p + 1))))
    checked = 0
    for s in scheds:
        assert T.valid(s)
        k_top = T.MAX_TIME // s[0]
        ks = [0, 1, 2, 63, 64, 1 << 20, (1 << 40) - 1, 1 << 40, k_top - 1, k_top]
        for seed in (0, 1, 0xDEADBEEFCAFEF00D, T.M64):
            for node in (0, 1, 65535, 2 ** 31 - 1):
                for k in ks:
                    if k < 0:
                        continue
                    rc, got = _due(L, s, seed, node, k)
                    if k > k_top:
                        assert rc == INVALID, (s, k)
                    else:
                        assert (rc, got) == (1, T.due(s, seed, node, k)), (s, seed, node, k)
                        checked += 1
    assert checked > 4000
    # times near 2^62: the last packet the rule reaches
    s = (1 << 22, (1 << 22) - 1, 1 << 22)
    rc, got = _due(L, s, 5, 9, 1 << 40)
    assert rc == 1 and got == T.due(s, 5, 9, 1 << 40) >= T.MAX_TIME
    assert _due(L, s, 5, 9, (1 << 40) + 1)[0] == INVALID
    # period 0: no packets; the refusals
    assert _due(L, (0, 0, 0), 1, 1, 0)[0] == 0
    assert _due(L, (100, 0, 0), 1, 1, -1)[0] == INVALID and _due(L, (100, 0, 0), 1, -1, 0)[0] == INVALID
    for bad in [(0, 1, 0), (0, 0, 1), (-1, 0, 0), (100, 100, 0), (100, -1, 0), (100, 0, 101), (100, 0, -1), ((1 << 40) + 1, 0, 0), (100, 0, 0, 1)]:
        assert not T.valid(bad) and _due(L, bad, 1, 1, 0)[0] == INVALID, bad
    out = C.c_int64()
    assert L.rm_traffic_due(None, 1, 1, 0, C.byref(out)) == INVALID
    rec = _lib.TrafficSchedule(100, 0, 0, 0)
    assert L.rm_traffic_due(C.byref(rec), 1, 1, 0, None) == INVALID
    assert rsa.Engine.traffic_due((100, 30, 0), 1, 2, 3) == 330 and rsa.Engine.traffic_due((0, 0, 0), 1, 2, 3) is None


def test_rm_traffic_validate_accepts_and_refuses_what_the_rule_says(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    V = rsa.Engine.traffic_validate
    good = [(100, 30, 0), (0, 0, 0), (1, 0, 1), (1 << 40, (1 << 40) - 1, 1 << 40), (100, 99, 100)]
    assert all(T.valid(s) for s in good)
    assert V(5, good) == OK and V(10, good, [9, 0, 0, 3, 9]) == OK      # a node may repeat: the last entry wins
    assert V(4, good) == INVALID and V(6, good) == INVALID              # without a list n has to be the node count
    assert V(10, good, [9, 0, 10, 3, 9]) == INVALID and V(10, good, [9, 0, -1, 3, 9]) == INVALID
    bad_records = [(0, 1, 0), (0, 0, 1), (-5, 0, 0), (100, 100, 0), (100, -1, 0), (100, 0, 101), (100, 0, -1), ((1 << 40) + 1, 0, 0)]
    for pos in (0, 2, 4):
        for bad in bad_records:
            assert not T.valid(bad)
            recs = list(good)
            recs[pos] = bad
            assert V(5, recs) == INVALID and V(10, recs, [1, 2, 3, 4, 5]) == INVALID, (pos, bad)
    recs = T.table_rows(good)
    recs[3, 3] = 1                                                       # reserved has to be 0
    assert not T.valid(tuple(recs[3])) and V(5, recs) == INVALID
    # NULL records with a count, negative counts; an empty list is fine
    idx = np.array([1, 2], dtype=np.int32)
    assert L.rm_traffic_validate(5, idx.ctypes.data, 2, None) == INVALID
    assert L.rm_traffic_validate(5, idx.ctypes.data, -1, recs.ctypes.data) == INVALID
    assert L.rm_traffic_validate(-1, idx.ctypes.data, 0, None) == INVALID
    assert L.rm_traffic_validate(5, idx.ctypes.data, 0, None) == OK and L.rm_traffic_validate(0, None, 0, None) == OK


def test_engine_takes_one_record_or_rows(rsa):
    """Engine's schedule argument: 2-D rows of three or four values, a structured array, or ONE record as a 1-D sequence"""
    tbl = rsa.Engine._traffic_table
    assert tbl((100, 30, 5)).view(np.int64).tolist() == [100, 30, 5, 0]
    assert tbl((100, 30, 5, 1)).view(np.int64).tolist() == [100, 30, 5, 1]           # (reserved is handed on for the library to refuse)
    assert tbl([(100, 30, 5), (7, 6, 7)]).view(np.int64).reshape(-1, 4).tolist() == [[100, 30, 5, 0], [7, 6, 7, 0]]
    assert tbl([(100, 30, 5, 0), (7, 6, 7, 9)]).view(np.int64).reshape(-1, 4).tolist() == [[100, 30, 5, 0], [7, 6, 7, 9]]
    assert tbl([]).shape == (0,) and tbl(np.zeros((0, 4), dtype=np.int64)).shape == (0,)
    assert tbl(tbl([(1, 0, 1)])).view(np.int64).tolist() == [1, 0, 1, 0]
    for bad in ((1, 2), (1, 2, 3, 4, 5, 6), [(1, 2), (3, 4)]):
        with pytest.raises(ValueError):
            tbl(bad)
    assert rsa.Engine.traffic_validate(1, (100, 30, 5)) == OK and rsa.Engine.traffic_validate(1, (100, 30, 5, 1)) == INVALID


# ---- 3. the host functions under the host sanitizers, in a stand-alone program -----------------------------------------------------

def test_host_functions_under_sanitizers(rsa, tmp_path):
    """tests/cpp/traffic_host_san_test.cpp with rm_api_traffic.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "traffic_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_traffic.cpp"), os.path.join(ROOT, "tests", "cpp", "traffic_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
