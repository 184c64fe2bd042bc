"""The reception stage's two rings where they wrap, fill and overflow (rm_events.hip: every `& pk_mask` / `& pool_mask`, the head
update of the finishing workgroup, the capacity tests of the append), the append on its own (k_ev_append) and a drain of more
fired groups than k_ev_emit stages in LDS -- on capacities of 64 packets and a few thousand links, 150 - 300 nodes.

Every drain's delivery list (order, destinations, rssi bits), the node state and rm_node_info_changed are held to the oracle's
serial event replay as in tests/test_gpu_events_batch.py (its Session), and the drain's return code, pending_packets and
oldest_packet to the host model of the rings (tests/events_ring_ref.py).  The scenes' conditions -- three wraps of either ring,
packets that straddle the pool's end, dropped ticks, exact fits, 2048 / 2050 groups -- are asserted from the model before anything
is compared (and without a GPU in tests/test_events_ring_ref.py)."""
import os

import numpy as np
import pytest

import events_ring_ref as R
from test_gpu_events_batch import Session, check_nodes, oracle_drain, run_plan, same_drain
from util import configure_engine, oracle_model, to_tx_records

pytestmark = pytest.mark.gpu

PLANS = {"lone": R.LONE_PLAN, "mixed": R.MIXED_PLAN}
OVERFLOW_PLAN = ("lone",) * R.OVERFLOW_TICKS


def _session(O, rsa, eng, scene, **more):
    seed, kind, params, kw = scene
    return Session(O, rsa, eng, seed, kind, params, **dict(kw, **more))


def _same_views(got, want, what):
    assert len(got) == len(want), "%s: %d drains, %d" % (what, len(got), len(want))
    for i, (x, y) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(x[0], y[0], err_msg="%s drain %d packets" % (what, i))
        np.testing.assert_array_equal(x[1], y[1], err_msg="%s drain %d destinations" % (what, i))
        np.testing.assert_array_equal(x[2].view(np.int64), y[2].view(np.int64), err_msg="%s drain %d rssi bits" % (what, i))
        assert x[3:] == y[3:], "%s drain %d (pending_packets, oldest_packet) %s, %s" % (what, i, x[3:], y[3:])


def _dropped_ticks_are_the_reported_drains(s, name):
    """the model's conditions hold, and the drains that returned RM_ERR_CAPACITY (Session.drain holds every drain's code to the
    model) were exactly the ones behind the dropped ticks"""
    rep = s.rings.report()
    R.overflow_conditions(rep, name, name)
    assert s.rings.reports == len(rep["dropped"]) == s.kept.count(False)
    assert len(s.views) == R.OVERFLOW_TICKS + 1


# ---------------------------------------------------------------- 1. the rings wrap
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("name", sorted(R.WRAP))
def test_rings_wrap(O, rsa, engine, name, plan):
    dry = R.wrap_traffic(O, name)
    run_plan(dry, PLANS[plan])
    R.wrap_conditions(dry.rings.report(), "%s, %s plan" % (name, plan))
    s = _session(O, rsa, engine, R.WRAP[name])
    assert run_plan(s, PLANS[plan]) == dry.delivered > 0
    assert s.rings.report() == dry.rings.report()
    assert len(s.views) == 121 + PLANS[plan].count("drain")


# ---------------------------------------------------------------- 2. fill, exact fit, overflow and recovery
@pytest.mark.parametrize("name", sorted(R.OVERFLOW))
def test_ring_overflows_and_recovers(O, rsa, engine, name):
    """a tick that does not fit is dropped whole and numbered, the drain behind it reports it once and still returns the other
    packets' deliveries, an exact fit is taken, and the rings take the next ticks again"""
    s = _session(O, rsa, engine, R.OVERFLOW[name])
    assert run_plan(s, OVERFLOW_PLAN) > 0
    _dropped_ticks_are_the_reported_drains(s, name)


def test_link_ring_overflows_in_a_batch(O, rsa, engine):
    """the link-ring scene as one batch of 60 ticks: the first reporting drain's code comes back, every view is filled and equal
    to the lone-tick run's"""
    lone = _session(O, rsa, engine, R.OVERFLOW["links"])
    run_plan(lone, OVERFLOW_PLAN)
    s = _session(O, rsa, engine, R.OVERFLOW["links"])
    assert run_plan(s, (R.OVERFLOW_TICKS,)) == lone.delivered > 0      # (Session.batch: the code, and every view against the oracle)
    _dropped_ticks_are_the_reported_drains(s, "links")
    _same_views(s.views, lone.views, "batch against lone ticks")


# ---------------------------------------------------------------- 3. the append on its own
def _kernels(eng):
    return {k.split("<")[0].strip() for k in eng.profile_kernels()}


@pytest.mark.parametrize("name", ["udgm_draws", "udgm_sources", "packets", "packets_sources"])
def test_append_on_its_own(O, rsa, engine, name):
    """rm_node_info between every tick and its drain, a normal call order of the radio-link server: bit for bit the same session.
    For the ticks named by source indices it changes the launches: their append waits for the drain and rides in its first launch
    (k_ev_append_select), and rm_node_info flushes it on its own (k_ev_append, every packet of the tick).  A tick of records
    appends at once either way."""
    what, plan = (R.WRAP[name], R.LONE_PLAN) if name in R.WRAP else (R.OVERFLOW[name], OVERFLOW_PLAN)
    # (RM_EV_FUSE=0, a developer knob: no append waits for the drain; it runs from the tick's call, which is not profiled)
    waits = name.endswith("_sources") and os.environ.get("RM_EV_FUSE") != "0"
    engine.profile_enable(1)
    plain = _session(O, rsa, engine, what)
    assert run_plan(plain, plan) > 0
    names = _kernels(engine)
    assert ("k_ev_append_select" in names) == waits and "k_ev_append" not in names, sorted(names)
    engine.profile_enable(1)
    s = _session(O, rsa, engine, what, info_between=True)
    assert run_plan(s, plan) == plain.delivered
    names = _kernels(engine)
    engine.profile_enable(0)
    assert "k_ev_append_select" not in names and "k_ev_select" in names and ("k_ev_append" in names) == waits, sorted(names)
    _same_views(s.views, plain.views, "rm_node_info between tick and drain")
    assert s.rings.report() == plain.rings.report()
    if name in R.OVERFLOW:
        _dropped_ticks_are_the_reported_drains(s, name)
    else:
        R.wrap_conditions(s.rings.report(), name)


# ---------------------------------------------------------------- 4. more groups in one drain than k_ev_emit stages
@pytest.mark.parametrize("P", R.GROUPS_P)
def test_groups_in_one_drain(O, rsa, engine, P):
    """2 P fired groups in one drain: 2048 fill the LDS key staging of k_ev_emit exactly, 2050 leave it (the rank pass reads
    global memory) and make the grid of 512 x 4 waves stride"""
    nodes, ticks, t_last = R.groups_script(O, P)
    configure_engine(engine, nodes, "udgm", {})
    engine._batch_reported = None
    engine.events_enable(*R.GROUPS_CAPACITY)
    engine.set_time(0)
    mdl = oracle_model(O, "udgm", {})
    sim = O.Sim(nodes.n)
    rings = R.Rings(*R.GROUPS_CAPACITY)
    base = 0
    for begin, end, pk in ticks:
        engine.tick(to_tx_records(rsa, pk), begin, end)
        want = O.tick(mdl, nodes, pk)
        assert rings.hand_over(begin, pk["start_us"], pk["air_us"], np.bincount(want.pkt, minlength=len(pk)))
        sim.medium_calls(want, pk, pkt_base=base)
        base += len(pk)
        got = engine.events_process(end)
        assert same_drain(got, oracle_drain(O, sim, end), "tick at %d" % begin) == 0
        model = rings.drain(end)
        assert (got[3], engine.oldest_pending_packet, 0) == (model[0], model[1], model[3])
    assert base == P == engine.events_next_packet()
    run_packet, run_first, run_count, dst, rssi, pending = engine.events_process(t_last, runs=True)
    model = rings.drain(t_last)
    assert model == (P, 0, False, 2 * P) and (pending, engine.oldest_pending_packet) == (P, 0)
    pkt, want_dst, want_rssi = oracle_drain(O, sim, t_last)
    assert len(run_packet) == len(np.unique(pkt)) > P // 2, "n_runs %d, packets that deliver %d" % (len(run_packet), len(np.unique(pkt)))
    assert len(dst) == len(pkt) > 4 * P
    assert run_first[0] == 0 and np.array_equal(run_first[1:], np.cumsum(run_count)[:-1]) and int(run_count.sum()) == len(dst)
    same_drain((np.repeat(run_packet, run_count), dst, rssi), (pkt, want_dst, want_rssi), "the drain of %d groups" % (2 * P))
    check_nodes(engine, sim, nodes, "after %d groups" % (2 * P))
    assert sim.pending == 0 and engine.events_process(t_last + 1)[3] == 0 and engine.oldest_pending_packet == P
    sim.close()
    engine.events_disable()
