"""Receiver listening schedules without a device: known answers of the listening rule, the library's
host export rm_listen_at against the reference (tests/listen_ref.py), and the conditions the scenes of tests/test_gpu_listen.py
have to meet -- asserted for the reference alone, so that no GPU test passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import errmodel_ref as R
import listen_ref as LR

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INVALID = -1


def test_known_answers_of_the_rule():
    on = LR.listening
    # period 0: always, whatever the time
    for t in (0, 1, -1, I64_MIN, I64_MAX, 3 * 10 ** 12):
        assert on((0, 0, 0), t)
    # on 0 never listens, on = period always does
    for t in (0, 49, 50, 51, 1049, -7, I64_MIN, I64_MAX):
        assert not on((1000, 0, 50), t)
        assert on((1000, 1000, 50), t)
        assert not on((1, 0, 0), t)
        assert on((1, 1, 0), t)
    s = (1000, 100, 50)
    assert on(s, 50)                    # t = phase: the window opens
    assert not on(s, 49)                # t = phase - 1: the last microsecond of the period before
    assert on(s, 50 + 100 - 1)          # the window's last microsecond
    assert not on(s, 50 + 100)          # ... and the first one after it
    assert on(s, 1050) and not on(s, 1049) and on(s, 1149) and not on(s, 1150)
    # negative times: C's remainder is negative there and is folded back into the period
    assert on(s, -950) and not on(s, -951) and on(s, -851) and not on(s, -850)
    assert on(s, -1000 * 10 ** 9 + 50) and not on(s, -1000 * 10 ** 9 + 49)
    # both ends of int64, where the subtraction wraps: d is computed modulo 2^64, not as an integer difference
    #   t = I64_MIN, phase = 1: the true difference is -2^63 - 1, the wrapped one is +2^63 - 1 = 9223372036854775807
    assert (I64_MAX % 1000) == 807
    assert not on((1000, 807, 1), I64_MIN) and on((1000, 808, 1), I64_MIN)
    #   t = I64_MAX, phase 0: no wrap, r = 807
    assert not on((1000, 807, 0), I64_MAX) and on((1000, 808, 0), I64_MAX)
    #   t = I64_MIN, phase 0: d = -2^63, C remainder -808, folded to 192
    assert not on((1000, 192, 0), I64_MIN) and on((1000, 193, 0), I64_MIN)
    #   the largest period: d = period gives r = 0; t = I64_MIN + 3 and phase = I64_MAX - 1 wrap to d = (2^63 + 3) - (2^63 - 2) = 5
    big = I64_MAX
    assert on((big, 1, 0), 0) and not on((big, 1, 0), 1) and on((big, 1, 0), big)
    assert not on((big, 5, big - 1), I64_MIN + 3) and on((big, 6, big - 1), I64_MIN + 3)
    # periods below and above 2^32
    p_lo, p_hi = (1 << 32) - 5, (1 << 32) + 7
    t = 3 * 10 ** 12
    for p in (p_lo, p_hi):
        r = (t - 11) % p
        assert not on((p, r, 11), t) and on((p, r + 1, 11), t)
        r = (-t - 11) % p   # (Python's % is the folded remainder for a negative dividend)
        assert not on((p, r, 11), -t) and on((p, r + 1, 11), -t)


def test_rule_equals_plain_integers_where_nothing_wraps():
    """listening() against floor-mod on unbounded integers, wherever t - phase fits int64 (there the wrap changes nothing)"""
    rng = np.random.default_rng(3)
    for _ in range(5000):
        period = int(rng.choice([1, 2, 1500, 125000, (1 << 32) - 1, 1 << 32, (1 << 40) + 3, I64_MAX]))
        on_us = int(rng.integers(0, period, endpoint=True))
        phase = int(rng.integers(0, period))
        t = int(rng.integers(I64_MIN, I64_MAX, endpoint=True))
        if not I64_MIN <= t - phase <= I64_MAX:
            continue
        assert LR.listening((period, on_us, phase), t) == ((t - phase) % period < on_us)


def _grid():
    times = [0, 1, -1, 49, 50, 51, 149, 150, 1049, 1050, -950, -951, 3 * 10 ** 12, -3 * 10 ** 12, I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1,
             (1 << 32) - 1, 1 << 32, (1 << 32) + 1, -(1 << 32), (1 << 31) - 1, 1 << 31]
    scheds = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1000, 0, 50), (1000, 1000, 50), (1000, 100, 50), (1000, 1, 999), (1500, 700, 1499),
              (125000, 1250, 77777), ((1 << 32) - 5, 1 << 31, 11), ((1 << 32) + 7, 1 << 31, (1 << 32) + 6), (1 << 32, 1, 0),
              (I64_MAX, 1, 0), (I64_MAX, I64_MAX, I64_MAX - 1), (I64_MAX, I64_MAX >> 1, I64_MAX - 1), (10_000_000, 1000, 9_000_000)]
    return [(s, t) for s in scheds for t in times]


def test_rm_listen_at_equals_the_reference():
    from radio_sim_amd import _lib
    L = _lib.lib()

    def at(s, t):
        rec = _lib.ListenSchedule(*s)
        return L.rm_listen_at(C.byref(rec), t)

    for s, t in _grid():
        assert at(s, t) == int(LR.listening(s, t)), (s, t)
    rng = np.random.default_rng(20261019)
    periods = [1, 2, 3, 1500, 2000, 3000, 7000, 125000, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 45) + 9, I64_MAX]
    seen = set()
    for k in range(10000):
        period = int(rng.choice(periods)) if k % 3 else int(rng.integers(1, I64_MAX, endpoint=True))
        s = (period, int(rng.integers(0, period, endpoint=True)), int(rng.integers(0, period)))
        if k % 4 == 0:
            t = int(rng.integers(I64_MIN, I64_MAX, endpoint=True))
        elif k % 4 == 1:
            t = int(rng.integers(-10 ** 13, 10 ** 13))
        else:
            t = s[2] + int(rng.integers(-3, 4)) * period + int(rng.choice([-1, 0, s[1] - 1, s[1]]))   # around the window's edges
            t = min(max(t, I64_MIN), I64_MAX)
        want = LR.listening(s, t)
        assert at(s, t) == int(want), (s, t)
        seen.add(want)
    assert seen == {True, False}


@pytest.mark.parametrize("bad", [(0, 1, 0), (0, 0, 1), (-1, 0, 0), (-1000, -1, -1), (1000, -1, 0), (1000, 1001, 0), (1000, 10, -1), (1000, 10, 1000),
                                 (I64_MIN, 0, 0)])
def test_rm_listen_at_refuses_a_bad_record(bad):
    from radio_sim_amd import _lib
    assert not LR.valid(bad)
    rec = _lib.ListenSchedule(*bad)
    for t in (0, 123456, -5):
        assert _lib.lib().rm_listen_at(C.byref(rec), t) == INVALID
    assert _lib.lib().rm_listen_at(None, 0) == INVALID


def test_apply_counts_what_sleep_alone_lost():
    """a hand-made tick: three frames, the links of one receiver asleep, one always on, one that was not delivered anyway"""
    class Res:
        pass
    w = Res()
    w.pkt = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    w.dst = np.array([1, 2, 1, 3, 1], dtype=np.int32)
    w.verdict = np.array([R.O.DELIVERED, R.O.DELIVERED, R.O.INTERFERED, R.O.DELIVERED, R.O.DELIVERED], dtype=np.uint8)
    new = np.zeros(3, dtype=R.O.PACKET_DTYPE)
    new["start_us"] = [0, 0, 500]
    sched = np.zeros(4, dtype=LR.DTYPE)
    sched[1] = (1000, 100, 450)   # awake in [450, 550): asleep at 0, awake at 500
    sched[3] = (1000, 0, 0)       # never
    after, missed = LR.apply(new, w, sched)
    np.testing.assert_array_equal(after, [R.O.INTERFERED, R.O.DELIVERED, R.O.INTERFERED, R.O.INTERFERED, R.O.DELIVERED])
    np.testing.assert_array_equal(missed, [0, 1, 0, 1])   # (the link that was interfered before counts nothing)


@pytest.mark.parametrize("name", ["lone", "serial", "batch", "batch_overlap"])
@pytest.mark.parametrize("em", [None, R.SEED], ids=["plain", "E10"])
def test_scene_conditions_hold_for_the_reference_alone(name, em):
    nd, lists, starts, air, sched, edges, runs, _ = LR.scene(name)
    assert set(edges) == set(LR.EDGES) and len(set(edges.values())) == len(LR.EDGES)
    assert max(starts) < min(s[2] for k, s in LR.EDGES.items() if k.startswith("neg"))   # d is negative at those two
    c = LR.conditions(runs[em], sched, edges)
    print(name, "error model", "on" if em is not None else "off", c)
    assert c["flipped"] >= 100
    assert c["kept_scheduled"] >= 100
    assert c["kept_always"] >= 100
    assert c["mixed"] >= 10
    assert all(v >= 1 for v in c["edges"].values()), c["edges"]
    assert int(runs[em].missed.sum()) == c["flipped"]
    # with every period 0 nothing changes
    zero = np.zeros(nd.n, dtype=LR.DTYPE)
    for w, new, before in zip(runs[em].res, runs[em].new, runs[em].before):
        after, missed = LR.apply(new, w, zero, before)
        np.testing.assert_array_equal(after, before)
        assert not missed.any()
