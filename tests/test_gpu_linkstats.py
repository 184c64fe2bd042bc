"""Watched-link statistics (rm_linkstats_*, rm_linkstats.hip) on the GPU.  Expected tables come from the
oracle through tests/linkstats_ref.py alone (tests/test_linkstats_ref.py holds the scenes' conditions for that reference).  Every
comparison is exact: equal integers, equal bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cca_batch_ref as BR
import csma_carry_ref as KR
import csma_ref as SR
import errmodel_ref as R
import linkstats_ref as K
import listen_ref as LR
import stats_ref as S
from test_gpu_cca import _bits, _engine as _plain_engine
from test_gpu_cca_batch import _refused
from test_gpu_csma import _csma
from test_gpu_csma_carry import _part
from test_gpu_stats import _launches, _lone, _run_batch, _same_links
from util import DeviceArray, assert_same, configure_engine, oracle_model, to_tx_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK = R.TICK
LINK_KERNELS = ("k_linkstats", "k_linkstats_batch", "k_linkstats_clear", "k_linkstats_scatter", "k_rows_gather", "k_rows_scatter")
INVALID, STATE = -1, -5


def _engine(rsa, nd, k=None, rows=None, params=R.PARAMS, em_seed=None, stats=False, sched=None, cap=None):
    eng = _plain_engine(rsa, nd, params, cap)
    if em_seed is not None:
        eng.set_error_model(rsa.EM_OQPSK_250K, seed=em_seed)
    if stats:
        eng.stats_enable()
    if sched is not None:
        eng.listen_set(sched)
    if k:
        eng.linkstats_enable(k)
        if rows is not None:
            eng.linkstats_watch(rows)
    return eng


def _check(eng, want, what, totals=True):
    """the engine's entries, peers and totals against the reference Table -> the entries"""
    tbl, tot = eng.linkstats_read()
    K.equal(tbl, want, what)
    np.testing.assert_array_equal(eng.linkstats_peers(), want.peer, err_msg=what + ": peers")
    if totals:
        assert tot == want.totals(), (what, tot, want.totals())
    return tbl


_REF = {}


def _ref(name, k, em=None):
    """a scene of listen_ref with its watch rows and its reference table, computed once, shared and left unchanged:
    -> (nd, lists, starts, air, sched, run, rows, Table after the whole run with the verdicts BEFORE E13 -- .after with em given)"""
    key = (name, k, em)
    if key not in _REF:
        nd, lists, starts, air, sched, _, runs, extra = LR.scene(name)
        run = runs[em]
        pairs = list(zip(run.new, run.res))
        rows = K.rows_first_heard(nd.n, k, pairs)
        want = K.table_of(nd.n, k, rows, pairs, run.before if em is None else run.after)[0]
        _REF[key] = (nd, lists, starts, air, sched, run, rows, want, extra)
    return _REF[key]


# ---- 1. every lone form on the SINR medium --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["flush", "view", "sources"])
def test_lone_forms(rsa, O, form):
    nd, lists, starts, air, _, run, rows, want, _ = _ref("lone", 4)
    srcs, start = lists[0], starts[0]
    on, off, d = _engine(rsa, nd, 4, rows), _engine(rsa, nd), DeviceArray(srcs)
    try:
        assert on.linkstats_enabled() == 4 and off.linkstats_enabled() == 0
        got, plain = _lone(on, form, d, srcs, start, air), _lone(off, form, d, srcs, start, air)
        _same_links(got, plain, form + ": watched links on against off")
        np.testing.assert_array_equal(got.dst, run.res[0].dst)
        np.testing.assert_array_equal(got.verdict, run.before[0])
        tbl = _check(on, want, form)
        assert want.totals() == {"ticks_counted": 1, "ticks_skipped": 0}
        idle = tbl["heard"] == 0
        assert idle.any() and (~idle).any()
        assert (tbl["first_start_us"][idle] == K.I64_MAX).all() and (tbl["last_start_us"][idle] == K.I64_MIN).all()
        assert (tbl["first_start_us"][~idle] == start).all() and (tbl["last_start_us"][~idle] == start).all()
    finally:
        d.free()
        on.close()
        off.close()


# ---- 2. rm_transmit packet by packet --------------------------------------------------------------------------------------

def test_transmit_packet_by_packet_on_the_sinr_medium(rsa, O):
    nd, lists, starts, air, _, run, rows, want, hex_len = _ref("serial", 4)
    on, off = _engine(rsa, nd, 4, rows), _engine(rsa, nd)
    try:
        for k, (l, s) in enumerate(zip(lists, starts)):
            a, b = on.transmit(int(l[0]), int(s), hex_len, cap=1 << 16), off.transmit(int(l[0]), int(s), hex_len, cap=1 << 16)
            assert a.count == b.count == run.res[k].count
            np.testing.assert_array_equal(a.dst, b.dst)
            np.testing.assert_array_equal(a.verdict, b.verdict)
            np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr))
            np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi))
        tbl = _check(on, want, "rm_transmit")
        hit = tbl["heard"] > 0
        assert len(np.unique(tbl["first_start_us"][hit])) >= 10   # every frame has its own start
    finally:
        on.close()
        off.close()


def test_transmit_on_udgm_consumes_the_draws_as_with_the_feature_off(rsa, O):
    """UDGM with rxProbability < 1, packet by packet through the general tick path: the links and the generator are the off run's
    (and the oracle's), and a medium without the sinr column leaves sinr_q8_sum at 0"""
    nd, kind, _, pk, _, seed = S.scene_udgm()
    params = {"udgm_success_ratio_rx": 0.7}
    hex_len = 254
    air = int(O.lib().orc_air_time_us(hex_len))
    srcs = pk["src"][:40]
    mdl = oracle_model(O, kind, params)
    state, pairs = O.lib().orc_jrandom_seed(seed), []
    for k, q in enumerate(srcs):
        new = nd.packets([int(q)], k * 5000, air)
        w = O.tick(mdl, nd, new, rng_state=state, cap=1 << 16)
        state = w.rng_state
        pairs.append((new, w))
    rows = K.rows_first_heard(nd.n, 4, pairs)
    want, matched, unmatched = K.table_of(nd.n, 4, rows, pairs, sinr=False)
    h, d = want.t["heard"], want.t["delivered"]
    assert matched >= 100 and ((h > 0) & (d == 0)).sum() >= 20 and (d > 0).sum() >= 20 and sum(int(w.pkt_draws.sum()) for _, w in pairs) > 0
    on, off = rsa.Engine(0), rsa.Engine(0)
    try:
        for eng in (on, off):
            configure_engine(eng, nd, kind, params)
            eng.seed(seed)
        on.linkstats_enable(4)
        on.linkstats_watch(rows)
        for k, q in enumerate(srcs):
            a, b = on.transmit(int(q), k * 5000, hex_len, cap=1 << 12), off.transmit(int(q), k * 5000, hex_len, cap=1 << 12)
            np.testing.assert_array_equal(a.dst, pairs[k][1].dst)
            np.testing.assert_array_equal(b.dst, pairs[k][1].dst)
            np.testing.assert_array_equal(a.verdict, pairs[k][1].verdict)
            np.testing.assert_array_equal(b.verdict, pairs[k][1].verdict)
            np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi))
        assert on.rng_state == off.rng_state == state
        tbl = _check(on, want, "rm_transmit on UDGM")
        assert not tbl["sinr_q8_sum"].any()
    finally:
        on.close()
        off.close()


# ---- 3. the dense tick on the Null medium ------------------------------------------------------------------------------------

def test_null_medium_through_the_dense_tick(rsa, O):
    scene = S.scene_null()
    nd, kind, params, pk, _, _ = scene
    cpu = S.oracle_tick(scene)
    rows = K.rows_first_heard(nd.n, 4, [(pk, cpu)])
    want, matched, unmatched = K.table_of(nd.n, 4, rows, [(pk, cpu)], sinr=False)
    assert matched >= 10000 and unmatched >= 5000
    srcs = np.ascontiguousarray(pk["src"], dtype=np.int32)
    on, off, d = rsa.Engine(0), rsa.Engine(0), DeviceArray(srcs)
    try:
        masks = []
        for eng in (on, off):
            configure_engine(eng, nd, kind, params)
            eng.set_link_capacity(1 << 20)
            if eng is on:
                eng.linkstats_enable(4)
                eng.linkstats_watch(rows)
            eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, S.AIR)
            if os.environ.get("RM_DENSE_TICK") != "0":   # (a run whose knobs never take the dense form has no masks to ask for)
                r = eng.result_dense()   # the masks still answer
                assert r.n_packets == len(srcs)
                cells = len(srcs) * r.chunks
                masks.append((r.chunks, r.rx_first, DeviceArray.read(r.cell_count, np.uint32, cells), DeviceArray.read(r.cell_mask, np.uint64, cells * 16)))
        if masks:
            assert masks[0][:2] == masks[1][:2]
            np.testing.assert_array_equal(masks[0][2], masks[1][2])
            np.testing.assert_array_equal(masks[0][3], masks[1][3])
            np.testing.assert_array_equal(masks[0][2].reshape(len(srcs), -1).sum(axis=1), np.bincount(cpu.pkt, minlength=len(srcs)))
        tbl = _check(on, want, "null, dense")
        assert not tbl["sinr_q8_sum"].any()
        assert_same(on.result_copy(len(srcs), cap=1 << 20), cpu, "null records")
    finally:
        d.free()
        on.close()
        off.close()


# ---- 4. batches of both SINR kinds: one batch, lone ticks, two batches ----------------------------------------------------------

@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("overlap", [False, True])
def test_batches_whole_tick_by_tick_and_split(rsa, O, overlap, k):
    nd, lists, starts, air, _, run, rows, want, _ = _ref("batch_overlap" if overlap else "batch", k)
    assert any(len(l) == 0 for l in lists) and any(w.count > 16384 for w in run.res) and any(w.count % 64 for w in run.res)
    a, b, c, dev = _engine(rsa, nd, k, rows), _engine(rsa, nd, k, rows), _engine(rsa, nd, k, rows), []
    try:
        _run_batch(a, lists, starts, air, dev)
        assert a.air_batch_stats()[0] == (1 if overlap else 0)
        one = _check(a, want, "one batch")
        for i, w in enumerate(run.res):   # the links are still the oracle's
            got = a.batch_result_copy(i, len(lists[i]), cap=1 << 20)
            assert got.count == w.count
            np.testing.assert_array_equal(got.dst, w.dst)
            np.testing.assert_array_equal(got.verdict, run.before[i])
        for l, s in zip(lists, starts):   # the same ticks one by one
            d = DeviceArray(l) if len(l) else None
            if d is not None:
                dev.append(d)
            _lone(b, "sources", d, l, s, air, t0=s)
        np.testing.assert_array_equal(_check(b, want, "lone ticks"), one)
        _run_batch(c, lists[:3], starts[:3], air, dev)   # two batches, cut at tick 3
        _run_batch(c, lists[3:], starts[3:], air, dev)
        np.testing.assert_array_equal(_check(c, want, "two batches"), one)
    finally:
        for d in dev:
            d.free()
        for e in (a, b, c):
            e.close()


# ---- 5. with the frame error model, the listening schedules and the traffic counters on -------------------------------------------

def _link_launches(eng):
    n, order = _launches(eng)
    return {name: v for name, v in n.items() if name in LINK_KERNELS}, n, order


@pytest.mark.parametrize("overlap", [False, True])
def test_all_four_passes_in_order(rsa, O, overlap):
    nd, lists, starts, air, sched, run, rows, want, _ = _ref("batch_overlap" if overlap else "batch", 4, R.SEED)
    plain = _ref("batch_overlap" if overlap else "batch", 4)[7]
    assert int(plain.t["delivered"].sum()) - int(want.t["delivered"].sum()) >= 100   # links E10 and E13 took: not delivered here
    np.testing.assert_array_equal(plain.t["heard"], want.t["heard"])
    on, off, dev = _engine(rsa, nd, 4, rows, em_seed=R.SEED, stats=True, sched=sched), _engine(rsa, nd, em_seed=R.SEED, stats=True, sched=sched), []
    try:
        for eng in (on, off):
            eng.profile_enable(1)
            _run_batch(eng, lists, starts, air, dev)
            eng.sync()
        seen, n, order = _link_launches(on)
        assert seen.get("k_linkstats_batch") == 1 and "k_linkstats" not in seen, (seen, order)
        assert n["k_errmodel_batch"] == n["k_listen_batch"] == n["k_stats_batch"] == 1
        assert order.index("k_errmodel_batch") < order.index("k_listen_batch") < order.index("k_stats_batch") < order.index("k_linkstats_batch"), order
        assert _link_launches(off)[0] == {}, _link_launches(off)
        _check(on, want, "E14 over the final verdicts")
        for i in range(len(lists)):
            np.testing.assert_array_equal(on.batch_result_copy(i, len(lists[i]), cap=1 << 20).verdict, run.after[i], err_msg="tick %d" % i)
        np.testing.assert_array_equal(on.stats_read()[0], off.stats_read()[0])
        assert on.stats_read()[1] == off.stats_read()[1]
        np.testing.assert_array_equal(on.listen_missed(), off.listen_missed())
        np.testing.assert_array_equal(on.listen_missed(), run.missed)
        _run_batch(on, lists, [s + 50 * TICK for s in starts], air, dev)   # one launch per batch
        on.sync()
        assert _link_launches(on)[0].get("k_linkstats_batch") == 2
    finally:
        for d in dev:
            d.free()
        on.close()
        off.close()


def test_lone_tick_with_all_four_passes(rsa, O):
    nd, lists, starts, air, sched, run, rows, want, _ = _ref("lone", 4, R.SEED)
    eng, d = _engine(rsa, nd, 4, rows, em_seed=R.SEED, stats=True, sched=sched), DeviceArray(lists[0])
    try:
        eng.profile_enable(1)
        got = _lone(eng, "sources", d, lists[0], starts[0], air)
        eng.sync()
        np.testing.assert_array_equal(got.verdict, run.after[0])
        seen, n, order = _link_launches(eng)
        assert seen.get("k_linkstats") == 1 and "k_linkstats_batch" not in seen, (seen, order)
        assert order.index("k_errmodel") < order.index("k_listen") < order.index("k_stats") < order.index("k_linkstats"), order
        _check(eng, want, "lone tick")
    finally:
        d.free()
        eng.close()


LONE_SWEEP = {"k_tick_frames", "k_tick_frames_sinr", "k_tick_frames_scan", "k_frames_cand", "k_filter", "k_filter_wg", "k_exact"}
BATCH_SWEEP = {"k_filter_wg_batch", "k_filter_wg_group", "k_exact_batch", "k_reorder_batch", "k_tick_frames_batch"}
LONE_PASSES = ("k_errmodel", "k_listen", "k_stats", "k_linkstats")
BATCH_PASSES = ("k_errmodel_batch", "k_listen_batch", "k_stats_batch", "k_linkstats_batch")


def test_batch_launched_tick_by_tick_with_all_four_passes(rsa, O):
    """a batch with an empty tick is launched one tick at a time (rm::batch_eligible wants frames in every tick): the four passes
    run once each over all its slots behind the last tick, in their order, and no lone tick's pass runs.  The scene's ticks are
    self-contained (a frame ends inside its tick), so the ticks that keep their lists have the whole batch's results."""
    nd, lists, starts, air, sched, run, rows, _, _ = _ref("batch", 4, R.SEED)
    gone = 4
    assert air <= TICK and len(lists[gone]) > 0
    lists = [l if i != gone else l[:0] for i, l in enumerate(lists)]
    kept = [i for i, l in enumerate(lists) if len(l)]
    assert len(kept) == 4
    want = K.table_of(nd.n, 4, rows, [(run.new[i], run.res[i]) for i in kept], [run.after[i] for i in kept])[0]
    counters, missed = S.Table(nd.n), np.zeros(nd.n, dtype=np.uint64)
    for i in kept:
        counters.add_result(run.new[i], run.res[i], verdict=run.after[i])
        missed += LR.apply(run.new[i], run.res[i], sched, run.before[i])[1]
    assert int(want.t["heard"].sum()) >= 1000 and int(missed.sum()) >= 100
    eng, dev = _engine(rsa, nd, 4, rows, em_seed=R.SEED, stats=True, sched=sched), []
    try:
        eng.profile_enable(1)
        _run_batch(eng, lists, starts, air, dev)
        eng.sync()
        n, order = _launches(eng)
        names = {k.split("<")[0].strip() for k in order}
        assert names & LONE_SWEEP and "k_store_ticks" in names and not names & BATCH_SWEEP, order   # the route: tick by tick
        assert [n.get(k) for k in BATCH_PASSES] == [1, 1, 1, 1] and not names & set(LONE_PASSES), (n, order)
        at = [order.index(k) for k in BATCH_PASSES]
        assert at == sorted(at) and all(at[0] > order.index(k) for k in order if k.split("<")[0].strip() in LONE_SWEEP), order
        _check(eng, want, "tick by tick")
        tbl, tot = eng.stats_read()
        S.equal(tbl, counters, "tick by tick")
        assert tot == counters.totals() == {"ticks_counted": len(kept), "ticks_skipped": 0}
        np.testing.assert_array_equal(eng.listen_missed(), missed)
        for i in kept:
            got = eng.batch_result_copy(i, len(lists[i]), cap=1 << 20)
            np.testing.assert_array_equal(got.dst, run.res[i].dst, err_msg="tick %d" % i)
            np.testing.assert_array_equal(got.verdict, run.after[i], err_msg="tick %d" % i)
    finally:
        for d in dev:
            d.free()
        eng.close()


_NULL = {}


def _null_ref():
    """the Null medium's scene under a schedule, computed once, shared and left unchanged:
    -> (nd, kind, params, pk, oracle result, sched, verdicts after E13, missed, watch rows)"""
    if not _NULL:
        scene = S.scene_null()
        nd, kind, params, pk, _, _ = scene
        cpu = S.oracle_tick(scene)
        sched, _ = LR.schedule(nd.n, LR.SCHED_SEED, LR.reached_receivers([(cpu, cpu.verdict)]))
        after, missed = LR.apply(pk, cpu, sched)
        _NULL["ref"] = (nd, kind, params, pk, cpu, sched, after, missed, K.rows_first_heard(nd.n, 4, [(pk, cpu)]))
    return _NULL["ref"]


def test_dense_lone_tick_with_the_three_counters(rsa, O):
    """the Null medium's tick ends with its cells' lane masks: the schedules', the counters' and the watched links' passes run over
    its records, once each and in this order, and rm_result_dense refuses a tick whose masks do not carry E13's verdicts"""
    nd, kind, params, pk, cpu, sched, after, missed, rows = _null_ref()
    want = K.table_of(nd.n, 4, rows, [(pk, cpu)], [after], sinr=False)[0]
    counters = S.Table(nd.n)
    counters.add_result(pk, cpu, verdict=after)
    assert 1000 <= int(missed.sum()) <= cpu.count - 1000 and int(want.t["delivered"].sum()) < int(want.t["heard"].sum())
    srcs = np.ascontiguousarray(pk["src"], dtype=np.int32)
    eng, d = rsa.Engine(0), DeviceArray(srcs)
    try:
        configure_engine(eng, nd, kind, params)
        eng.set_link_capacity(1 << 20)
        eng.stats_enable()
        eng.listen_set(sched)
        eng.linkstats_enable(4)
        eng.linkstats_watch(rows)
        eng.profile_enable(1)
        eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, S.AIR)
        eng.sync()
        n, order = _launches(eng)
        if os.environ.get("RM_DENSE_TICK") != "0":   # (a run whose knobs never take the dense form sweeps as any other medium)
            assert any(k.startswith("k_dense_count") for k in order), order
        assert [n.get(k) for k in LONE_PASSES[1:]] == [1, 1, 1] and "k_errmodel" not in n and not set(BATCH_PASSES) & set(n), (n, order)
        assert order.index("k_listen") < order.index("k_stats") < order.index("k_linkstats"), order
        _refused(rsa, eng, STATE, eng.result_dense)
        _check(eng, want, "null, dense, three passes")
        tbl, tot = eng.stats_read()
        S.equal(tbl, counters, "null, dense, three passes")
        assert tot == {"ticks_counted": 1, "ticks_skipped": 0}
        np.testing.assert_array_equal(eng.listen_missed(), missed)
        got = eng.result_copy(len(srcs), cap=1 << 20)
        np.testing.assert_array_equal(got.dst, cpu.dst)
        np.testing.assert_array_equal(got.verdict, after)
    finally:
        d.free()
        eng.close()


def test_refusal_precedence_with_all_four_on(rsa, O):
    """a receiver partition with every pass on: the forms that ask about the frame error model name it first; a lone tick's entry
    point asks about the three others before the tick reaches the SINR medium's own path, and names the counters.  Nothing is
    launched and no table moves."""
    nd, lists, starts, air, sched, run, rows, _, _ = _ref("lone", 4, R.SEED)
    srcs = lists[0]
    eng, d = _engine(rsa, nd, 4, rows, em_seed=R.SEED, stats=True, sched=sched), DeviceArray(srcs)
    recs = DeviceArray(to_tx_records(rsa, nd.packets(srcs, 100 * TICK, air)))
    try:
        _lone(eng, "sources", d, srcs, starts[0], air)   # (the tables hold something to lose)
        links, counters, missed = eng.linkstats_read(), eng.stats_read(), eng.listen_missed()
        assert links[0]["heard"].any() and counters[0]["rx_heard"].any() and missed.any()
        t = 100 * TICK

        def refused(what, call, begins):
            eng.profile_enable(1)
            msg = _refused(rsa, eng, STATE, call)
            assert msg.startswith("rm error %d: %s: " % (STATE, begins)), (what, msg)
            eng.sync()
            assert eng.profile_kernels() == {}, (what, eng.profile_kernels())
            for got, was in zip(eng.linkstats_read() + eng.stats_read(), links + counters):
                assert (got == was) if isinstance(was, dict) else np.array_equal(got, was), what
            np.testing.assert_array_equal(eng.listen_missed(), missed, err_msg=what)

        eng.set_partition(0, nd.n // 2)
        refused("a batch", lambda: eng.batch_run_sources_device([t], [t + TICK], [d.ptr.value], [len(srcs)], [t], [air]),
                "the frame error model is on")
        refused("records on the SINR medium", lambda: eng.tick_run_records_device(t, t + TICK, recs.ptr.value, len(srcs), t + air),
                "the frame error model is on")
        refused("sources on the SINR medium", lambda: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air),
                "statistics are on")
        eng.set_partition(0, nd.n)
        eng.set_model(1)   # a reference medium: the three counters stay on
        assert eng.stats_enabled() and eng.listen_enabled() and eng.linkstats_enabled() == 4
        eng.set_partition(0, nd.n // 2)
        refused("sources on a reference medium", lambda: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air),
                "statistics are on")
    finally:
        recs.free()
        d.free()
        eng.close()


def test_off_launches_nothing(rsa, O):
    nd, lists, starts, air, _, run, rows, want, _ = _ref("batch", 4)
    eng, dev, d = _engine(rsa, nd, 4, rows), [], DeviceArray(lists[0])
    try:
        eng.linkstats_enable(0)
        assert eng.linkstats_enabled() == 0
        _refused(rsa, eng, STATE, eng.linkstats_read)
        eng.profile_enable(1)
        _run_batch(eng, lists, starts, air, dev)
        _lone(eng, "sources", d, lists[0], 60 * TICK, air, t0=60 * TICK)
        eng.sync()
        seen, _, order = _link_launches(eng)
        assert seen == {}, (seen, order)
    finally:
        d.free()
        for x in dev:
            x.free()
        eng.close()


# ---- 6. gated and CSMA-CA: whole and split --------------------------------------------------------------------------------------

def test_csma_whole_and_split_give_identical_tables(rsa, O):
    sc = BR.scene(O, "multi")
    n_ticks, p = SR.SCENES["multi"]
    r = SR.run(O, "multi")
    n = sc.nd.n
    pairs = [(e.new, e.raw) for e in r.exp[:n_ticks] if e.raw is not None]
    rows = K.rows_first_heard(n, 4, pairs)
    want, matched, unmatched = K.table_of(n, 4, rows, pairs)
    h = want.t["heard"]
    assert matched >= 1000 and unmatched >= 100 and (h >= 2).sum() >= 50 and ((want.t["delivered"] > 0) & (want.t["delivered"] < h)).sum() >= 10
    assert (want.t["last_start_us"][h >= 2] > want.t["first_start_us"][h >= 2]).any()
    t_cca = [sc.times(i)[1] for i in range(n_ticks)]
    tables = []
    for cuts in ((), (6,), (3, 9)):
        eng = _engine(rsa, sc.nd, 4, rows, sc.params)
        try:
            edges, carry = [0] + list(cuts) + [n_ticks], None
            for first, last in zip(edges[:-1], edges[1:]):
                want_carry, _ = KR.carry_at(r, first, t_cca)
                carry = want_carry[:0] if carry is None else carry
                _, _, _, carry = _part(rsa, eng, sc, r.lists[first:last], first, "device", sc.threshold, p, carry)
            tables.append(_check(eng, want, "cuts %s" % (cuts,), totals=False))
            assert eng.linkstats_read()[1]["ticks_skipped"] == 0
        finally:
            eng.close()
    np.testing.assert_array_equal(tables[0], tables[1])
    np.testing.assert_array_equal(tables[0], tables[2])
    # ... and the whole as ONE CSMA-CA batch (E8's own entry point)
    eng = _engine(rsa, sc.nd, 4, rows, sc.params)
    try:
        _csma(rsa, eng, sc, r.lists, 0, "device", sc.threshold, p)
        np.testing.assert_array_equal(_check(eng, want, "one CSMA-CA batch", totals=False), tables[0])
    finally:
        eng.close()


def test_gated_lone_ticks_and_one_gated_batch_agree(rsa, O):
    import cca_ref as CR
    from test_gpu_cca_batch import _batch as _gated_batch
    sc = BR.scene(O, "multi")
    r = BR.run(O, "multi", 12)
    n = sc.nd.n
    pairs = [(e.new, e.raw) for e in r.exp[:12] if e.raw is not None]
    rows = K.rows_first_heard(n, 4, pairs)
    want, matched, _ = K.table_of(n, 4, rows, pairs)
    assert matched >= 1000
    tables = []
    for way in ("lone", "batch"):
        eng = _engine(rsa, sc.nd, 4, rows, sc.params)
        try:
            if way == "lone":
                for i in range(12):
                    t0, tc, ts = sc.times(i)
                    eng.tick_run_sources_cca(t0, t0 + CR.TICK, r.lists[i], ts, CR.AIR, tc, sc.threshold)
            else:
                _gated_batch(eng, sc, r.lists[:12], 0, "device", sc.threshold)
            tables.append(_check(eng, want, "gated " + way, totals=False))
        finally:
            eng.close()
    np.testing.assert_array_equal(tables[0], tables[1])


# ---- 7. watch semantics and the tables' lifetime -------------------------------------------------------------------------------------

def test_a_peer_switch_clears_only_its_slot(rsa, O):
    """half of `batch`, then one peer changed in each of 100 rows (a parent switch), then the rest: kept slots carry on, changed slots
    count from their clear"""
    nd, lists, starts, air, _, run, rows, _, _ = _ref("batch", 4)
    pairs = list(zip(run.new, run.res))
    want = K.Table(nd.n, 4)
    want.watch(None, rows)
    for i in range(3):
        want.add(pairs[i][0], pairs[i][1], run.before[i])
    # the switch: a node whose slot has counted drops that peer for a source it hears later and does not watch yet
    later = {}
    for new, w in pairs[3:]:
        for q, j in zip(w.pkt.tolist(), w.dst.tolist()):
            later.setdefault(j, []).append(int(new["src"][q]))
    idx, new_rows = [], []
    for j in range(nd.n):
        counted = np.flatnonzero(want.t["heard"][j] > 0)
        fresh = [s for s in later.get(j, []) if s not in rows[j] and s != j]
        if len(counted) and fresh:
            row = rows[j].copy()
            row[counted[0]] = fresh[0]
            idx.append(j)
            new_rows.append(row)
        if len(idx) == 100:
            break
    assert len(idx) == 100
    idx, new_rows = np.array(idx[::-1], dtype=np.int32), np.array(new_rows[::-1], dtype=np.int32)   # (a list in no particular order)
    eng, dev = _engine(rsa, nd, 4, rows), []
    try:
        _run_batch(eng, lists[:3], starts[:3], air, dev)
        before = _check(eng, want, "first half")
        eng.linkstats_watch(new_rows, idx)
        want.watch(idx, new_rows)
        mid = _check(eng, want, "after the switch")
        changed = mid["heard"] != before["heard"]
        assert changed.sum() == 100 and (mid["heard"][changed] == 0).all() and (mid["first_start_us"][changed] == K.I64_MAX).all()
        np.testing.assert_array_equal(eng.linkstats_peers(idx), new_rows)
        part, tot = eng.linkstats_read(idx)
        np.testing.assert_array_equal(part, mid[idx])
        _run_batch(eng, lists[3:], starts[3:], air, dev)
        for i in range(3, len(pairs)):
            want.add(pairs[i][0], pairs[i][1], run.before[i])
        end = _check(eng, want, "second half")
        assert (end["heard"][changed] > 0).sum() >= 100   # the new peers are heard
        kept = ~changed & (before["heard"] > 0)
        assert (end["heard"][kept] > before["heard"][kept]).sum() >= 100   # kept slots carry on from their history
        # rm_linkstats_reset keeps the peers and clears entries and totals
        eng.linkstats_reset()
        want.reset()
        _check(eng, want, "reset")
        assert eng.linkstats_read()[1] == {"ticks_counted": 0, "ticks_skipped": 0}
        # the same K again changes nothing; another K starts empty
        eng.linkstats_enable(4)
        _check(eng, want, "the same K again")
        eng.linkstats_enable(2)
        assert eng.linkstats_enabled() == 2
        _check(eng, K.Table(nd.n, 2), "another K")
        _refused(rsa, eng, INVALID, lambda: eng.linkstats_enable(3))
        _refused(rsa, eng, INVALID, lambda: eng.linkstats_enable(16))
        assert eng.linkstats_enabled() == 2
    finally:
        for d in dev:
            d.free()
        eng.close()


def test_lifetime_across_medium_and_node_changes(rsa, O):
    nd, lists, starts, air, _, run, rows, one, _ = _ref("lone", 4)
    srcs, w = lists[0], run.res[0]
    eng, d = _engine(rsa, nd), DeviceArray(srcs)
    want, far, clock = K.Table(nd.n, 4), 100 * TICK, [0]
    want.watch(None, rows)

    def tick():
        t = clock[0]
        clock[0] += far
        _lone(eng, "sources", d, srcs, t, air, t0=t)
        want.add(LR.packets(nd, srcs, t, air), w, run.before[0])

    try:
        for call in (eng.linkstats_read, eng.linkstats_peers, eng.linkstats_reset, eng.linkstats_device, lambda: eng.linkstats_watch(rows)):
            _refused(rsa, eng, STATE, call)   # before the first enable
        eng.linkstats_enable(4)
        _check(eng, K.Table(nd.n, 4), "fresh tables")
        eng.linkstats_watch(rows)
        tick()
        tick()
        tbl = _check(eng, want, "two ticks add up")
        hit = tbl["heard"] > 0
        assert (tbl["first_start_us"][hit] == 0).all() and (tbl["last_start_us"][hit] == far).all()
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
        eng.seed(3)
        i = int(srcs[0])
        eng.update_node(i, float(nd.x[i]), float(nd.y[i]), float(nd.z[i]), float(nd.txpower[i]), int(nd.channel[i]), 1, 1.0, 1.0)
        eng.upload_table(nd)
        assert eng.linkstats_enabled() == 4
        _check(eng, want, "rm_set_model / rm_seed / rm_node_update / rm_nodes_upload with the same count")
        tick()
        _check(eng, want, "counting goes on")
        # another node count switches the feature off
        half = O.NodeTable(nd.n // 2)
        half.x, half.y = nd.x[:nd.n // 2], nd.y[:nd.n // 2]
        eng.upload_table(half)
        assert eng.linkstats_enabled() == 0
        _refused(rsa, eng, STATE, eng.linkstats_read)
        eng.linkstats_enable(8)
        _check(eng, K.Table(nd.n // 2, 8), "enabled again on the smaller table")
    finally:
        d.free()
        eng.close()


# ---- 8. a slot over its link capacity -----------------------------------------------------------------------------------------------

def test_a_slot_over_the_link_capacity_counts_nothing(rsa, O):
    """test_gpu_stats' batch: a tick of 150 frames one link over the capacity and two small ticks that survive"""
    nd, lists, starts, air, sched, _, _, _ = LR.scene("batch")[:8]
    lists, starts = [lists[3], lists[4][:3], lists[5][:2]], starts[3:]
    run = LR.Run(nd, lists, starts, air, np.zeros(nd.n, dtype=LR.DTYPE))
    cap = run.res[0].count - 1
    assert cap > 16384 and all(0 < 16 * w.count < cap for w in run.res[1:])
    pairs = list(zip(run.new, run.res))
    rows = K.rows_first_heard(nd.n, 4, pairs)
    want = K.Table(nd.n, 4)
    want.watch(None, rows)
    want.skip()
    for i in (1, 2):
        assert want.add(pairs[i][0], pairs[i][1], run.before[i])[0] > 0
    whole = K.table_of(nd.n, 4, rows, pairs, run.before)[0]
    assert int(whole.t["heard"].sum()) > int(want.t["heard"].sum()) + 1000
    eng, dev = _engine(rsa, nd, 4, rows, cap=cap), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        assert [bool(eng.batch_result_count(i)[1]) for i in range(3)] == [True, False, False]
        _check(eng, want, "batch with one dropped tick")
        assert eng.linkstats_read()[1] == {"ticks_counted": 2, "ticks_skipped": 1}
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_as_it_was(rsa, O):
    from radio_sim_amd import _lib
    nd, lists, starts, air, _, run, rows, _, _ = _ref("lone", 4)
    srcs, w = lists[0], run.res[0]
    eng, d = _engine(rsa, nd, 4, rows), DeviceArray(srcs)
    want, clock = K.Table(nd.n, 4), [0]
    want.watch(None, rows)
    try:
        def plain(what):
            """a plain lone tick is the reference's (the window is unharmed) and adds exactly its own links"""
            t = clock[0]
            clock[0] += 100 * TICK
            got = _lone(eng, "sources", d, srcs, t, air, t0=t)
            np.testing.assert_array_equal(got.dst, w.dst, err_msg=what)
            np.testing.assert_array_equal(got.verdict, run.before[0], err_msg=what)
            np.testing.assert_array_equal(_bits(got.sinr), _bits(w.sinr), err_msg=what)
            want.add(LR.packets(nd, srcs, t, air), w, run.before[0])
            _check(eng, want, what)

        def refused(what, call, partition=None, code=STATE):
            t = clock[0]
            state = eng.rng_state
            if partition:
                partition()
            _refused(rsa, eng, code, lambda: call(t))
            if partition:
                eng.set_partition(0, nd.n)
            _check(eng, want, what + ": tables untouched")
            assert eng.rng_state == state and eng.linkstats_enabled() == 4, what
            plain(what)

        def flush(t):
            eng.tick_begin(t, t + TICK)
            eng.enqueue_tx(int(srcs[0]), t, air)
            eng.tick_flush(cap=1 << 16)

        plain("to begin with")
        half = lambda: eng.set_partition(0, nd.n // 2)   # noqa: E731
        refused("a lone tick on a partition", lambda t: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air), half)
        refused("a lone tick on a spatial partition", lambda t: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air),
                lambda: eng.set_partition_spatial(0, 2))
        refused("a batch on a partition", lambda t: eng.batch_run_sources_device([t], [t + TICK], [d.ptr.value], [len(srcs)], [t], [air]), half)
        refused("rm_tick_flush on a partition", flush, half)
        refused("rm_transmit on a partition", lambda t: eng.transmit(int(srcs[0]), t, 254, cap=1 << 16), half)
        refused("gathered sources", lambda t: eng.batch_run_gathered_sources_device([t], [t + TICK], d.ptr.value, 1, len(srcs), [t], air))
        refused("rm_dist_batch", lambda t: eng.dist_batch_run_sources_device([t], [t + TICK], d.ptr.value, len(srcs), [t], air))
        refused("rm_dist_tick", lambda t: eng.dist_tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air))
        # invalid rows: the whole list is validated before anything changes
        j0, j1 = 10, 11
        good = np.array([[1, 2, 3, -1], [5, 6, -1, 7]], dtype=np.int32)
        for what, bad_rows, idx in [("own node", [[1, 2, 3, -1], [5, j1, -1, 7]], [j0, j1]),
                                    ("a repeated peer", [[1, 2, 3, -1], [5, 6, -1, 5]], [j0, j1]),
                                    ("a repeated node", good, [j0, j0]),
                                    ("a peer out of range", [[1, 2, 3, -1], [5, 6, -1, nd.n]], [j0, j1]),
                                    ("a peer below -1", [[1, 2, 3, -1], [5, 6, -2, 7]], [j0, j1]),
                                    ("a node out of range", good, [j0, nd.n]),
                                    ("a negative node", good, [-1, j1])]:
            refused(what, lambda t, r=bad_rows, i=idx: eng.linkstats_watch(r, i), code=INVALID)
        refused("no list, another count", lambda t: eng.linkstats_watch(rows[:-1]), code=INVALID)
        for idx in ([0, nd.n], [-1, 0]):
            refused("read %s" % idx, lambda t, idx=idx: eng.linkstats_read(np.array(idx, dtype=np.int32)), code=INVALID)
            refused("peers %s" % idx, lambda t, idx=idx: eng.linkstats_peers(np.array(idx, dtype=np.int32)), code=INVALID)
        L = _lib.lib()
        out = np.zeros((nd.n, 4), dtype=rsa.LINK_STATS_DTYPE)
        assert L.rm_linkstats_watch(eng._h, None, nd.n, None) == INVALID and L.rm_linkstats_watch(None, None, 0, None) == INVALID
        assert L.rm_linkstats_read(eng._h, None, nd.n, None, None) == INVALID and L.rm_linkstats_read(eng._h, None, nd.n - 1, out.ctypes.data, None) == INVALID
        assert L.rm_linkstats_read(eng._h, None, -1, out.ctypes.data, None) == INVALID and L.rm_linkstats_peers_get(eng._h, None, nd.n, None) == INVALID
        assert L.rm_linkstats_enable(None, 4) == INVALID and L.rm_linkstats_reset(None) == INVALID and L.rm_linkstats_device(None, None, None, None) == INVALID
        assert L.rm_linkstats_enabled(None) == 0
        plain("after the invalid calls")
        # a reference medium too (its ticks take other entry points)
        eng.set_model(1)
        eng.set_partition(0, nd.n // 2)
        _refused(rsa, eng, STATE, lambda: flush(clock[0]))
        _refused(rsa, eng, STATE, lambda: eng.tick_run_sources_device(clock[0], clock[0] + TICK, d.ptr.value, len(srcs), clock[0], air))
        _refused(rsa, eng, STATE, lambda: eng.transmit(int(srcs[0]), clock[0], 254, cap=1 << 16))
        eng.set_partition(0, nd.n)
        _check(eng, want, "after the refusals on a reference medium")
        # rm_group_*: a member with watched links refuses the group's tick (a group of one too); off again, the group's tick runs
        grp = rsa.Group([0])
        try:
            grp.upload_table(nd)
            grp.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
            member = L.rm_group_context(grp._h, 0)
            tbl = np.ascontiguousarray(rows)
            assert L.rm_linkstats_enable(member, 4) == 0 and L.rm_linkstats_enabled(member) == 4
            assert L.rm_linkstats_watch(member, None, nd.n, tbl.ctypes.data) == 0
            recs = to_tx_records(rsa, nd.packets(srcs, 0, air))
            _refused(rsa, grp, STATE, lambda: grp.tick(recs, 0, TICK, cap=1 << 20))
            tot = _lib.StatsTotals()
            assert L.rm_linkstats_read(member, None, nd.n, out.ctypes.data, tot) == 0
            assert not out["heard"].any() and (out["first_start_us"] == K.I64_MAX).all() and tot.ticks_counted == 0
            assert L.rm_linkstats_enable(member, 0) == 0 and L.rm_linkstats_enabled(member) == 0
            got = grp.tick(recs, 0, TICK, cap=1 << 20)
            assert got.count == w.count
            np.testing.assert_array_equal(got.verdict, run.before[0])
        finally:
            grp.close()
    finally:
        d.free()
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
        eng.linkstats_enable(4)
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        assert eng.linkstats_enabled() == 0
        eng.linkstats_enable(0)
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_enable_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs: the pass is not part of them"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)


# ---- 10. the device pointers and the list reads ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_device_pointers_and_list_reads(rsa, O, k):
    nd, lists, starts, air, _, run, rows, want, _ = _ref("lone", k)
    eng, d = _engine(rsa, nd, k, rows), DeviceArray(lists[0])
    try:
        _lone(eng, "sources", d, lists[0], starts[0], air)
        tbl = _check(eng, want, "K = %d" % k)
        p_peer, p_tbl, p_tot = eng.linkstats_device()
        np.testing.assert_array_equal(DeviceArray.read(p_peer, np.int32, nd.n * k).reshape(nd.n, k), rows)
        np.testing.assert_array_equal(DeviceArray.read(p_tbl, rsa.LINK_STATS_DTYPE, nd.n * k).reshape(nd.n, k), tbl)
        np.testing.assert_array_equal(DeviceArray.read(p_tot, np.uint64, 2), [1, 0])
        idx = np.array([int(lists[0][3]), 0, nd.n - 1, int(run.res[0].dst[0]), int(lists[0][3])], dtype=np.int32)   # (a read may name a node twice)
        part, tot = eng.linkstats_read(idx)
        np.testing.assert_array_equal(part, tbl[idx])
        assert tot == {"ticks_counted": 1, "ticks_skipped": 0}
        big = np.random.default_rng(1).integers(0, nd.n, 5000).astype(np.int32)
        np.testing.assert_array_equal(eng.linkstats_read(big)[0], tbl[big])
        np.testing.assert_array_equal(eng.linkstats_peers(big), rows[big])
        # a list watch directly behind a list read, and a list read directly behind it: one host-mapped block serves both
        some = np.unique(big)[:700].astype(np.int32)
        empty = np.full((len(some), k), -1, dtype=np.int32)
        eng.linkstats_watch(empty, some)
        want2 = K.Table(nd.n, k)
        want2.peer[...], want2.t[...] = want.peer, want.t
        want2.counted = want.counted
        want2.watch(some, empty)
        np.testing.assert_array_equal(eng.linkstats_read(big)[0], want2.t[big])
        _check(eng, want2, "after emptying 700 rows")
    finally:
        d.free()
        eng.close()
