"""The host model of the reception stage's rings (tests/events_ring_ref.py) on hand-made ticks, and the conditions of every scene
of tests/test_gpu_events_rings.py -- wraps, packets that straddle the pool's end, dropped ticks, exact fits, group counts -- as
the oracle plus the model see them.  These are conditions of the inputs.  No GPU."""
import numpy as np
import pytest

import events_ring_ref as R
from test_gpu_events_batch import run_plan


# ---------------------------------------------------------------- the rule, on ticks written out by hand
def _tick(rings, now, packets, **kw):
    """packets: [(start, air, links)]"""
    return rings.hand_over(now, [p[0] for p in packets], [p[1] for p in packets], [p[2] for p in packets], **kw)


def test_exact_fit_is_accepted_and_one_more_is_not():
    r = R.Rings(64, 128)
    assert _tick(r, 0, [(0, 5000, 1)] * 60)
    assert r.drain(1000)[:3] == (60, 0, False)
    assert _tick(r, 1000, [(1000, 5000, 1)] * 4)             # 60 + 4 == 64
    assert r.exact_fit == {"packets": 1, "links": 0}
    assert r.drain(2000)[:3] == (64, 0, False)
    assert not _tick(r, 2000, [(2000, 10, 0)])               # 64 + 1 > 64
    assert r.dropped == [(2, "packets")] and r.next_packet == 65
    assert r.drain(3000)[:3] == (64, 0, True)                # reported by the drain that follows ...
    assert r.drain(3001)[:3] == (64, 0, False)               # ... once
    # the link ring: 64 links pending, 64 more fit exactly, one more does not
    r = R.Rings(64, 128)
    assert _tick(r, 0, [(0, 5000, 32)] * 2) and _tick(r, 0, [(0, 5000, 64)])
    assert r.exact_fit == {"packets": 0, "links": 1}
    assert not _tick(r, 0, [(0, 10, 1)]) and r.dropped == [(2, "links")]
    assert not _tick(r, 0, [(0, 10, 1)] * 62) and r.dropped[-1] == (3, "both")
    assert _tick(r, 0, [(0, 10, 0)])                         # (a packet nobody hears needs no link)


def test_heads_move_lazily_and_one_long_frame_holds_the_ring():
    r = R.Rings(64, 128)
    assert _tick(r, 0, [(0, 100, 3), (0, 100000, 5), (10, 100, 7)])
    assert r.drain(1000) == (3, 0, False, 5)                 # both short frames are finished by this drain ...
    assert r.drain(2000) == (2, 1, False, 0)                 # ... and the one at the head is released by the next
    assert (r.head, r.pool_head) == (1, 3)
    assert _tick(r, 2000, [(1990, 10, 2)])                   # (a start before "now" is clamped: t1 = 2010)
    assert r.drain(3000) == (3, 1, False, 2)
    assert r.drain(200000) == (3, 1, False, 1)               # the long frame ends: the ring empties one drain later
    assert r.drain(200001) == (0, 4, False, 0)
    assert (r.head, r.tail, r.pool_head, r.pool_tail) == (4, 4, 17, 17)
    assert not _tick(r, 200001, [(0, 1, 1)] * 65) and r.drain(200002) == (0, 69, True, 0)   # a dropped tick keeps its numbers


def test_immediate_packets_padding_and_straddles():
    r = R.Rings(64, 64)
    assert _tick(r, 0, [(0, 100000, 30), (0, 100000, 30)], immediate=True)
    assert r.drain(1) == (2, 0, False, 2)                    # the constant-loss medium: delivered at once, released a drain later
    assert not _tick(r, 1, [(1, 10, 5)]) and r.drain(2) == (0, 3, True, 0)   # (until then its links fill the pool)
    assert _tick(r, 2, [(2, 10, 10), (1, 10, 0), (2, 10, 9)], padding=[False, True, False])
    assert r.straddles == 1                                  # links 60 .. 69 of a ring of 64
    assert r.drain(5) == (3, 3, False, 2) and r.pool_head == 60
    assert r.drain(100) == (3, 3, False, 2)
    assert r.drain(101) == (0, 6, False, 0)
    rep = r.report()
    assert rep["link_wraps"] == 79 / 64 and rep["max_links"] == 60 and rep["max_packets"] == 3


def test_capacities_round_up_to_powers_of_two_from_64():
    assert [R.pow2_at_least(v) for v in (0, 1, 64, 65, 512, 1000)] == [64, 64, 64, 128, 512, 1024]
    assert (R.Rings(10, 100).pk_cap, R.Rings(10, 100).pool_cap) == (64, 128)


# ---------------------------------------------------------------- the scenes' conditions
def test_plans():
    assert R.plan_ticks(R.LONE_PLAN) == R.plan_ticks(R.MIXED_PLAN) == 120
    assert 64 in R.MIXED_PLAN and "lone" in R.MIXED_PLAN and "drain" in R.MIXED_PLAN


@pytest.mark.parametrize("plan", ["lone", "mixed"])
@pytest.mark.parametrize("name", sorted(R.WRAP))
def test_wrap_scene(O, name, plan):
    t = R.wrap_traffic(O, name)
    assert (t.rings.pk_cap, t.rings.pool_cap) == t.capacity and t.rings.pk_cap == 64
    assert run_plan(t, R.LONE_PLAN if plan == "lone" else R.MIXED_PLAN) > 0
    rep = t.rings.report()
    R.wrap_conditions(rep, "%s, %s plan" % (name, plan))
    assert len(t.kept) == 120 and all(t.kept)
    assert rep["max_packets"] < 64                           # (the wrap scenes leave the fill to the overflow scenes)


def test_null_scene_links_per_packet(O):
    t = R.wrap_traffic(O, "null")
    _, _, pk = t._next_tick()
    while not len(pk):
        _, _, pk = t._next_tick()
    want = O.tick(t.mdl, t.nodes, pk)
    cnt = np.bincount(want.pkt, minlength=len(pk))
    assert cnt.min() >= 146 and cnt.max() <= 149             # 150 nodes, 3 disabled: three rounds of 64 lanes per packet


@pytest.mark.parametrize("name", sorted(R.OVERFLOW))
def test_overflow_scene(O, name):
    t = R.overflow_traffic(O, name)
    run_plan(t, ("lone",) * R.OVERFLOW_TICKS)
    rep = t.rings.report()
    R.overflow_conditions(rep, name, name)
    assert t.rings.reports == len(rep["dropped"]) == t.kept.count(False)
    assert t.rings.next_packet == t.base                     # the dropped ticks' packets were numbered


@pytest.mark.parametrize("P", R.GROUPS_P)
def test_group_counts(O, P):
    nodes, ticks, t_last = R.groups_script(O, P)
    assert sum(len(pk) for _, _, pk in ticks) == P and 28 <= len(ticks) <= 32
    r = R.Rings(*R.GROUPS_CAPACITY)
    mdl = O.model(1)
    for begin, end, pk in ticks:
        assert len(np.unique(pk["src"])) == len(pk)
        want = O.tick(mdl, nodes, pk)
        assert r.hand_over(begin, pk["start_us"], pk["air_us"], np.bincount(want.pkt, minlength=len(pk)))
        assert end <= pk["start_us"].min()
        assert r.drain(end)[3] == 0                          # nothing fires at the tick ends
    pending, oldest, reported, groups = r.drain(t_last)
    assert (pending, oldest, reported) == (P, 0, False)
    assert groups == 2 * P and groups == {1024: 2048, 1025: 2050}[P]
    assert r.drain(t_last + 1) == (0, P, False, 0)
    assert not r.dropped and r.max_links <= r.pool_cap
