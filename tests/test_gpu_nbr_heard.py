"""The heard form of the source cache: where no draw can happen a context keeps, per source node, the FINISHED
records of its frames -- receiver node index, rssi, verdict, in node order -- and a later batch copies them to the frame's place
in the ordered records (k_reorder_served_batch) instead of sweeping, evaluating and ranking the frame again.  Nothing of it may
show in the results: every tick of every batch here is held to the oracle bit for bit (heard set, order, rssi, verdict), with
the lists being filled from the ordered records, with frames served from them, and across the changes of form."""
import numpy as np
import pytest

import stats_ref as S
from util import configure_engine, oracle_model, random_nodes, assert_same, DeviceArray

pytestmark = pytest.mark.gpu

AIR = 8128
SERVED = "k_reorder_served_batch"


@pytest.fixture(autouse=True, params=[None, "2"], ids=["", "near-lists"])
def near_lists(request, monkeypatch):
    """Every case twice: the filter the sizes here choose (256 shards per tick), and the 1024-receiver workgroups with the
    near-frame lists that the bench shape takes (64 shards per tick)."""
    if request.param:
        monkeypatch.setenv("RM_NEAR_LISTS", request.param)
        monkeypatch.setenv("RM_WG_RPT", "4")


def _layout(O, n, seed, side=None):
    return random_nodes(O, n, side if side else 50.0 * np.sqrt(np.pi * n / 20.0), seed=seed)


def _run(engine, srcs):
    dev = [DeviceArray(s) for s in srcs]
    starts = [1000 * b for b in range(len(srcs))]
    engine.batch_run_sources_device(starts, [s + 1000 for s in starts], [d.ptr.value for d in dev], [len(s) for s in srcs], starts,
                                    [AIR] * len(srcs))
    for d in dev:
        d.free()
    return starts


def _batch(engine, O, nd, mdl, srcs, state, what):
    """one launch sequence over the ticks `srcs`; every tick against the oracle; -> (generator state, oracle results)"""
    starts = _run(engine, srcs)
    want = []
    for b, s in enumerate(srcs):
        cpu = O.tick(mdl, nd, nd.packets(s, start_us=starts[b], air_us=AIR), rng_state=state)
        state = cpu.rng_state
        assert_same(engine.batch_result_copy(b, len(s)), cpu, "%s, tick %d" % (what, b))
        assert engine.batch_result_count(b) == (cpu.count, 0)
        want.append(cpu)
    assert engine.rng_state == state
    return state, want


def _ticks(n, n_ticks, per_tick, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, per_tick, replace=False)).astype(np.int32) for _ in range(n_ticks)]


def _push(engine, nd, i):
    engine.update_node(int(i), nd.x[i], nd.y[i], nd.z[i], nd.txpower[i], int(nd.channel[i]), int(nd.enabled[i]), nd.rxprob[i], nd.txprob[i])


def _served_launches(engine):
    return sum(v[0] for k, v in engine.profile_kernels().items() if k.startswith(SERVED))


def _swept(engine, n_slots):
    """per slot: the candidates the sweep handed to the exact stage (rm_slot_stats: swept frames only -- 0 with heard links
    means every frame of the tick was served from a list)"""
    return [engine.slot_stats(b)[0] for b in range(n_slots)]


CASES = [
    ("udgm", {}),
    ("udgm_const", {}),
    ("logdist", dict(ld_sigma_db=0.0)),
    ("logdist", dict(ld_sigma_db=4.0, ld_seed=11)),
]


@pytest.mark.parametrize("kind,params", CASES)
def test_served_records(engine, rsa, O, kind, params):
    """The same ticks three times, then known and new sources mixed, so that a wave's 64 frames interleave served and swept
    ones.  The served kernel is launched in every draw-free batch (and copies from the second repetition on).  The candidates
    form over the same kind of scene, never launching it, is test_form_switch's middle step: the library has no environment
    knob that forces it (every knob it reads needs a row in tests/test_gpu_variants.py)."""
    n = 6000
    nd = _layout(O, n, seed=5)
    configure_engine(engine, nd, kind, params)
    engine.profile_enable(1)
    engine.seed(77)
    state = O.lib().orc_jrandom_seed(77)
    mdl = oracle_model(O, kind, params)
    srcs = _ticks(n, 5, 150, seed=3)
    first = None
    for rep in range(3):
        state, want = _batch(engine, O, nd, mdl, srcs, state, "%s, batch %d" % (kind, rep))
        assert all(w.count > 0 for w in want)
        swept = _swept(engine, len(srcs))
        if rep == 0:
            first = swept
            assert all(c >= w.count for c, w in zip(swept, want)), swept     # every frame swept: candidates cover the heard links
        else:
            assert swept == [0] * len(srcs), (rep, swept)                    # every frame served: nothing swept, links all there
    assert _served_launches(engine) > 0, sorted(engine.profile_kernels())
    mixed = [np.unique(np.concatenate([s[::2], t])).astype(np.int32) for s, t in zip(srcs, _ticks(n, 5, 90, seed=4))]
    state, _ = _batch(engine, O, nd, mdl, mixed, state, "%s, mixed batch" % kind)
    swept = _swept(engine, len(mixed))
    assert all(0 < c < f for c, f in zip(swept, first)), (swept, first)      # the new sources only
    state, _ = _batch(engine, O, nd, mdl, mixed, state, "%s, mixed batch again" % kind)
    assert _swept(engine, len(mixed)) == [0] * len(mixed)
    ran = engine.profile_kernels()
    assert SERVED in ran, sorted(ran)
    for k in ("k_nc_claim_batch", "k_nc_fill_batch", "k_nc_expand_batch"):
        assert any(name.startswith(k) for name in ran), (k, sorted(ran))


def test_list_lengths_in_one_tick(engine, rsa, O):
    """A third of the sources reaches nobody (an empty list is a valid hit), a few strong ones have more than 64 and fewer than
    1024 heard links: the served copy spans several 64-lane rounds, and zero-length frames sit between long ones in a wave."""
    n = 6000
    nd = _layout(O, n, seed=21)
    rng = np.random.default_rng(22)
    srcs = _ticks(n, 4, 180, seed=23)
    every = np.unique(np.concatenate(srcs))
    nd.txpower[every[rng.random(len(every)) < 1.0 / 3.0]] = -30.0
    strong = np.concatenate([s[5::40] for s in srcs])
    nd.txpower[strong] = 16.0
    params = dict(ld_sigma_db=2.0, ld_seed=5)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    engine.profile_enable(1)
    engine.seed(9)
    state = O.lib().orc_jrandom_seed(9)
    for rep in range(3):    # filled, then served twice
        state, want = _batch(engine, O, nd, mdl, srcs, state, "batch %d" % rep)
    for b, w in enumerate(want):
        per_pkt = np.bincount(w.pkt, minlength=len(srcs[b]))
        assert (per_pkt == 0).sum() >= 30 and ((per_pkt > 64) & (per_pkt < 1024)).sum() >= 3 and per_pkt.max() < 1024, (b, np.sort(per_pkt)[-8:])
        z = np.flatnonzero(per_pkt == 0)     # zero-length frames inside a wave's 64 frames, not only at the tick's ends
        assert np.any((z > 0) & (z < len(per_pkt) - 1))
    assert _served_launches(engine) > 0


def test_the_verdict_column(engine, rsa, O):
    """txprob = 0 on some sources: no draw is possible (the tick is not stochastic), every link of theirs is RM_INTERFERED --
    the verdict is part of a list, not a constant."""
    n = 6000
    nd = _layout(O, n, seed=31)
    srcs = _ticks(n, 4, 160, seed=32)
    dead = np.concatenate([s[::3] for s in srcs])
    nd.txprob[dead] = 0.0
    for kind, params in (("udgm", {}), ("logdist", dict(ld_sigma_db=4.0, ld_seed=7))):
        configure_engine(engine, nd, kind, params)
        mdl = oracle_model(O, kind, params)
        engine.profile_enable(1)
        engine.seed(5)
        state = O.lib().orc_jrandom_seed(5)
        for rep in range(3):    # filled, then served twice
            state, want = _batch(engine, O, nd, mdl, srcs, state, "%s, batch %d" % (kind, rep))
        v = np.concatenate([w.verdict for w in want])
        assert (v == O.INTERFERED).sum() > 100 and (v == O.DELIVERED).sum() > 100
        assert _served_launches(engine) > 0


def test_dropped_ticks_leave_no_list(engine, rsa, O):
    """A link capacity below one tick's heard total: the tick is reported dropped in both runs (its records stop at the
    capacity, so the fill leaves it alone: nothing of it may be served later), nothing crashes; with room again the same batch
    equals the oracle twice -- swept where no list was left, served elsewhere.  rm_set_link_capacity does not move the cache's
    epoch: the lists of the ticks that fitted stay valid across both changes of the capacity, so the last two runs serve them.
    The sweep's candidate counts (rm_slot_stats) say which frames were swept: the dropped tick's loud sources every time until
    a run with room has filled their lists, the other ticks' sources in the very first run only."""
    n = 6000
    nd = _layout(O, n, seed=41)
    params = dict(ld_sigma_db=0.0)
    mdl = oracle_model(O, "logdist", params)
    small = _ticks(n, 4, 150, seed=42)
    loud = np.setdiff1d(_ticks(n, 1, 260, seed=43)[0], np.concatenate(small))[:200].astype(np.int32)
    nd.txpower[np.concatenate(small)] = -14.0   # a few links per frame: a tick of them fits every candidate shard 20 times over
    nd.txpower[loud] = 10.0
    big = np.unique(np.concatenate([small[0][::2], small[2][::2], loud])).astype(np.int32)   # half of two ticks' sources, and loud ones
    srcs = [small[0], small[1], big, small[2], small[3]]
    configure_engine(engine, nd, "logdist", params)
    starts = [1000 * b for b in range(len(srcs))]
    want = [O.tick(mdl, nd, nd.packets(s, start_us=starts[b], air_us=AIR)) for b, s in enumerate(srcs)]
    cap = 1 << 14
    assert 20 * max(w.count for b, w in enumerate(want) if b != 2) < cap < want[2].count
    engine.set_link_capacity(cap)
    engine.profile_enable(1)
    for rep in range(2):
        _run(engine, srcs)
        for b, s in enumerate(srcs):
            cnt, dropped = engine.batch_result_count(b)
            assert dropped == (1 if b == 2 else 0), (rep, b)
            if b != 2:
                assert_same(engine.batch_result_copy(b, len(s)), want[b], "small capacity, batch %d, tick %d" % (rep, b))
        swept = _swept(engine, len(srcs))
        assert swept[2] > 0 and all((c > 0) == (rep == 0) for b, c in enumerate(swept) if b != 2), (rep, swept)
    engine.set_link_capacity(1 << 20)
    state = engine.rng_state                 # (no draw happens: the generator stays where it is)
    for rep in range(2):
        _batch(engine, O, nd, mdl, srcs, state, "room again, batch %d" % rep)
        swept = _swept(engine, len(srcs))
        # the dropped tick left no list: its loud sources are swept once more; the lists of the others outlived both capacities
        assert (swept[2] > 0) == (rep == 0) and all(c == 0 for b, c in enumerate(swept) if b != 2), (rep, swept)
    assert _served_launches(engine) > 0


def test_form_switch(engine, rsa, O):
    """Draw-free (heard form), then receivers whose links draw (candidates form, the generator's state compared), then
    draw-free again: twice at each step, all against the oracle."""
    n = 6000
    nd = _layout(O, n, seed=51)
    params = dict(ld_sigma_db=4.0, ld_seed=11)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    srcs = _ticks(n, 4, 170, seed=52)
    engine.profile_enable(1)
    engine.seed(21)
    state = O.lib().orc_jrandom_seed(21)
    for rep in range(2):
        state, _ = _batch(engine, O, nd, mdl, srcs, state, "draw-free, batch %d" % rep)
    served = _served_launches(engine)
    assert served > 0
    lossy = np.random.default_rng(53).choice(n, n // 5, replace=False)
    nd.rxprob[lossy[:40]] = 0.6
    for i in lossy[:40]:
        _push(engine, nd, i)
    before = state
    for rep in range(2):
        state, want = _batch(engine, O, nd, mdl, srcs, state, "receivers that draw, batch %d" % rep)
    assert state != before                          # draws were consumed
    assert _served_launches(engine) == served       # the candidates form
    nd.rxprob[lossy[:40]] = 1.0
    for i in lossy[:40]:
        _push(engine, nd, i)
    for rep in range(2):
        state, _ = _batch(engine, O, nd, mdl, srcs, state, "draw-free again, batch %d" % rep)
    assert _served_launches(engine) > served


def test_readers_of_served_slots(engine, rsa, O):
    """The traffic counters (E11) over three batches, the last two served, equal three batches' oracle-derived counters; the
    packed host block of a fully served batch equals the per-slot copies."""
    n = 6000
    nd = _layout(O, n, seed=61)
    srcs = _ticks(n, 4, 150, seed=62)
    nd.txprob[np.concatenate([s[::7] for s in srcs])] = 0.0
    params = dict(ld_sigma_db=4.0, ld_seed=3)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    engine.stats_enable()
    engine.profile_enable(1)
    table = S.Table(n)
    engine.seed(4)
    state = O.lib().orc_jrandom_seed(4)
    for rep in range(3):
        state, want = _batch(engine, O, nd, mdl, srcs, state, "batch %d" % rep)
        for b, w in enumerate(want):
            table.add_result(nd.packets(srcs[b], start_us=1000 * b, air_us=AIR), w)
    tbl, tot = engine.stats_read()
    S.equal(tbl, table, "three batches, two of them served")
    assert tot == table.totals()
    assert _served_launches(engine) > 0
    views, status = engine.batch_result_view(len(srcs))
    assert status == [0] * len(srcs)
    for b, s in enumerate(srcs):
        got = engine.batch_result_copy(b, len(s))
        v = views[b]
        assert v.count == got.count == want[b].count
        for col in ("pkt", "dst", "verdict", "rssi"):
            np.testing.assert_array_equal(getattr(v, col), getattr(got, col), err_msg="tick %d, %s" % (b, col))
        assert_same(v, want[b], "host block, tick %d" % b)
