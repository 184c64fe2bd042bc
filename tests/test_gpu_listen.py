"""Receiver listening schedules (rm_listen_*, rm_listen.hip) on the GPU.  Expected verdicts and missed
counts come from the oracle through tests/listen_ref.py alone (tests/test_listen_ref.py holds the scenes' conditions for that
reference).  Every comparison is exact: equal bytes, equal bits, equal integers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cca_batch_ref as BR
import cca_ref as CR
import csma_carry_ref as KR
import csma_ref as SR
import errmodel_ref as R
import listen_ref as LR
import stats_ref as S
from test_gpu_cca import _bits, _engine as _plain_engine
from test_gpu_cca_batch import _batch as _gated_batch, _refused
from test_gpu_csma import _csma
from test_gpu_csma_carry import _part
from test_gpu_stats import _launches, _lone, _run_batch, _same_links
from util import DeviceArray, configure_engine, oracle_model, to_tx_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK = R.TICK
LISTEN_KERNELS = ("k_listen", "k_listen_batch", "k_rows_gather", "k_rows_scatter")
INVALID, STATE = -1, -5
UC_INTERFERED, UC_DELIVERED = 3, 4


def _engine(rsa, nd, sched=None, params=R.PARAMS, em_seed=None, stats=False, cap=None):
    eng = _plain_engine(rsa, nd, params, cap)
    if em_seed is not None:
        eng.set_error_model(rsa.EM_OQPSK_250K, seed=em_seed)
    if stats:
        eng.stats_enable()
    if sched is not None:
        eng.listen_set(sched)
    return eng


def _same_but_verdict(a, b, what):
    """two engine results: everything but the verdict column bit for bit"""
    assert a.count == b.count, (what, a.count, b.count)
    for f in ("dst", "pkt_offset", "pkt_interference"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg="%s: %s" % (what, f))
    np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr), err_msg=what + ": sinr")


# ---- 1. every lone form on the SINR medium --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["flush", "view", "sources"])
def test_lone_forms(rsa, O, form):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("lone")
    run, srcs, start = runs[None], lists[0], starts[0]
    on, off, zero, d = _engine(rsa, nd, sched), _engine(rsa, nd), _engine(rsa, nd, np.zeros(nd.n, dtype=LR.DTYPE)), DeviceArray(srcs)
    try:
        assert on.listen_enabled() and zero.listen_enabled() and not off.listen_enabled()
        got, plain, allon = (_lone(e, form, d, srcs, start, air) for e in (on, off, zero))
        _same_but_verdict(got, plain, form + ": schedules on against off")
        np.testing.assert_array_equal(got.dst, run.res[0].dst)
        np.testing.assert_array_equal(plain.verdict, run.before[0])
        np.testing.assert_array_equal(got.verdict, run.after[0])
        np.testing.assert_array_equal(on.listen_missed(), run.missed)
        _same_links(allon, plain, form + ": every period 0 against off")
        assert not zero.listen_missed().any()
    finally:
        d.free()
        for e in (on, off, zero):
            e.close()


# ---- 2. rm_transmit packet by packet --------------------------------------------------------------------------------------

def test_transmit_packet_by_packet_on_the_sinr_medium(rsa, O):
    nd, lists, starts, air, sched, _, runs, hex_len = LR.scene("serial")
    run = runs[None]
    on, off = _engine(rsa, nd, sched), _engine(rsa, nd)
    try:
        for k, (l, s) in enumerate(zip(lists, starts)):
            a, b = on.transmit(int(l[0]), int(s), hex_len, cap=1 << 16), off.transmit(int(l[0]), int(s), hex_len, cap=1 << 16)
            assert a.count == b.count == run.res[k].count
            np.testing.assert_array_equal(a.dst, b.dst)
            np.testing.assert_array_equal(a.dst, run.res[k].dst)
            np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr))
            np.testing.assert_array_equal(b.verdict, run.before[k])
            np.testing.assert_array_equal(a.verdict, run.after[k])
        np.testing.assert_array_equal(on.listen_missed(), run.missed)
    finally:
        on.close()
        off.close()


def test_transmit_on_udgm_consumes_the_draws_as_with_the_feature_off(rsa, O):
    """UDGM with rxProbability < 1, packet by packet: the verdicts before E13 are the oracle's (java.util.Random walked as ever), the
    ones after it the reference's, and the generator ends where the off run's does"""
    nd, kind, _, pk, _, seed = S.scene_udgm()
    params = {"udgm_success_ratio_rx": 0.7}
    hex_len = 254
    air = int(O.lib().orc_air_time_us(hex_len))
    srcs = pk["src"][:40]
    mdl = oracle_model(O, kind, params)
    state, cpu, news = O.lib().orc_jrandom_seed(seed), [], []
    for k, q in enumerate(srcs):
        new = nd.packets([int(q)], k * 5000, air)
        w = O.tick(mdl, nd, new, rng_state=state, cap=1 << 16)
        state = w.rng_state
        cpu.append(w)
        news.append(new)
    sched, _ = LR.schedule(nd.n, LR.SCHED_SEED, LR.reached_receivers((w, w.verdict) for w in cpu))
    on, off = rsa.Engine(0), rsa.Engine(0)
    try:
        for eng in (on, off):
            configure_engine(eng, nd, kind, params)
            eng.seed(seed)
        on.listen_set(sched)
        missed, flipped, draws = np.zeros(nd.n, dtype=np.uint64), 0, 0
        for k, q in enumerate(srcs):
            a, b = on.transmit(int(q), k * 5000, hex_len, cap=1 << 12), off.transmit(int(q), k * 5000, hex_len, cap=1 << 12)
            after, m = LR.apply(news[k], cpu[k], sched)
            np.testing.assert_array_equal(b.dst, cpu[k].dst)
            np.testing.assert_array_equal(b.verdict, cpu[k].verdict)
            np.testing.assert_array_equal(a.dst, cpu[k].dst)
            np.testing.assert_array_equal(a.verdict, after)
            np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi))
            missed += m
            flipped += int((after != cpu[k].verdict).sum())
            draws += int(cpu[k].pkt_draws.sum())
        assert flipped >= 20 and draws > 0
        assert on.rng_state == off.rng_state == state
        np.testing.assert_array_equal(on.listen_missed(), missed)
    finally:
        on.close()
        off.close()


# ---- 3. batches of both SINR kinds; one launch per batch, none when off ---------------------------------------------------------

def _listen_launches(eng):
    n, order = _launches(eng)
    return {k: v for k, v in n.items() if k in LISTEN_KERNELS}, order


@pytest.mark.parametrize("overlap", [False, True])
def test_batches_of_both_kinds(rsa, O, overlap):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("batch_overlap" if overlap else "batch")
    run = runs[None]
    eng, dev = _engine(rsa, nd, sched), []
    try:
        eng.profile_enable(1)
        _run_batch(eng, lists, starts, air, dev)
        eng.sync()
        seen, order = _listen_launches(eng)
        assert seen == {"k_listen_batch": 1}, (seen, order)
        assert eng.air_batch_stats()[0] == (1 if overlap else 0)
        for k, w in enumerate(run.res):
            got = eng.batch_result_copy(k, len(lists[k]), cap=1 << 20)
            assert got.count == w.count
            np.testing.assert_array_equal(got.dst, w.dst)
            np.testing.assert_array_equal(_bits(got.sinr), _bits(w.sinr))
            np.testing.assert_array_equal(got.verdict, run.after[k], err_msg="tick %d" % k)
        np.testing.assert_array_equal(eng.listen_missed(), run.missed)
        # after rm_listen_clear: the off run's verdicts, and no kernel of rm_listen.hip
        eng.listen_clear()
        assert not eng.listen_enabled()
        far = [s + 50 * TICK for s in starts]
        _run_batch(eng, lists, far, air, dev)
        eng.sync()
        assert _listen_launches(eng)[0] == {"k_listen_batch": 1}   # (the count of the whole context: still the first batch's one)
        if not overlap:   # (self-contained ticks: the same verdicts at any time)
            for k, w in enumerate(run.res):
                np.testing.assert_array_equal(eng.batch_result_copy(k, len(lists[k]), cap=1 << 20).verdict, run.before[k])
    finally:
        for d in dev:
            d.free()
        eng.close()


@pytest.mark.parametrize("mode", ["never set", "cleared"])
def test_off_launches_nothing(rsa, O, mode):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("batch")
    eng, dev, d = _engine(rsa, nd), [], DeviceArray(lists[0])
    try:
        eng.profile_enable(1)
        if mode == "cleared":
            eng.listen_set(sched)
            eng.listen_clear()
        _run_batch(eng, lists, starts, air, dev)
        _lone(eng, "sources", d, lists[0], 60 * TICK, air, t0=60 * TICK)
        eng.sync()
        seen, order = _listen_launches(eng)
        assert seen == {}, (seen, order)
        np.testing.assert_array_equal(eng.batch_result_copy(0, len(lists[0]), cap=1 << 20).verdict, runs[None].before[0])
    finally:
        d.free()
        for x in dev:
            x.free()
        eng.close()


# ---- 4. with the frame error model and the traffic counters on -----------------------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
def test_error_model_first_then_schedules_then_counters(rsa, O, overlap):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("batch_overlap" if overlap else "batch")
    run, plain = runs[R.SEED], runs[None]
    assert int(plain.missed.sum()) - int(run.missed.sum()) >= 100   # links E10 took first: not counted as missed
    want = S.Table(nd.n)
    for new, w, after in zip(run.new, run.res, run.after):
        want.add_result(new, w, verdict=after)
    eng, dev = _engine(rsa, nd, sched, em_seed=R.SEED, stats=True), []
    try:
        eng.profile_enable(1)
        _run_batch(eng, lists, starts, air, dev)
        eng.sync()
        n, order = _launches(eng)
        assert n["k_errmodel_batch"] == n["k_listen_batch"] == n["k_stats_batch"] == 1
        assert order.index("k_errmodel_batch") < order.index("k_listen_batch") < order.index("k_stats_batch"), order
        for k in range(len(lists)):
            np.testing.assert_array_equal(eng.batch_result_copy(k, len(lists[k]), cap=1 << 20).verdict, run.after[k], err_msg="tick %d" % k)
        S.equal(eng.stats_read()[0], want, "E11 over the final verdicts")
        np.testing.assert_array_equal(eng.listen_missed(), run.missed)
    finally:
        for d in dev:
            d.free()
        eng.close()


def test_lone_tick_with_error_model_and_counters(rsa, O):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("lone")
    run = runs[R.SEED]
    want = S.Table(nd.n)
    want.add_result(run.new[0], run.res[0], verdict=run.after[0])
    eng, d = _engine(rsa, nd, sched, em_seed=R.SEED, stats=True), DeviceArray(lists[0])
    try:
        got = _lone(eng, "sources", d, lists[0], starts[0], air)
        np.testing.assert_array_equal(got.verdict, run.after[0])
        S.equal(eng.stats_read()[0], want, "lone tick")
        np.testing.assert_array_equal(eng.listen_missed(), run.missed)
    finally:
        d.free()
        eng.close()


# ---- 5. split independence --------------------------------------------------------------------------------------------------

_MULTI = {}


def _multi(O):
    """cca_ref's scene `multi` as the gates run it (cca_batch_ref, 12 ticks) and as CSMA-CA runs it (csma_ref), one schedule for both"""
    if not _MULTI:
        sc = BR.scene(O, "multi")
        gated, csma = BR.run(O, "multi", 12), SR.run(O, "multi")
        pairs = [(e.raw, e.raw.verdict) for r in (gated, csma) for e in r.exp if e.raw is not None]
        sched, _ = LR.schedule(sc.nd.n, LR.SCHED_SEED, LR.reached_receivers(pairs))
        _MULTI.update(sc=sc, gated=gated, csma=csma, sched=sched)
    return _MULTI["sc"], _MULTI["gated"], _MULTI["csma"], _MULTI["sched"]


def _exp_after(exp, sched, n):
    """a tick's cca_ref.Expected under the schedules -> (verdict column, missed, {(src, start, dst): verdict})"""
    if exp.raw is None:
        return np.zeros(0, dtype=np.uint8), np.zeros(n, dtype=np.uint64), {}
    v, m = LR.apply(exp.new, exp.raw, sched)
    pk = exp.new[exp.raw.pkt]
    return v, m, {(int(s), int(t), int(d)): int(x) for s, t, d, x in zip(pk["src"], pk["start_us"], exp.raw.dst, v)}


def _check_links(gpu, exp, verdict, what):
    assert gpu.count == exp.count, (what, gpu.count, exp.count)
    np.testing.assert_array_equal(gpu.pkt, exp.pkt, err_msg=what + ": pkt")
    np.testing.assert_array_equal(gpu.dst, exp.dst, err_msg=what + ": dst")
    np.testing.assert_array_equal(gpu.verdict, verdict, err_msg=what + ": verdict")
    np.testing.assert_array_equal(_bits(gpu.sinr), _bits(exp.sinr), err_msg=what + ": sinr")


def test_gated_lone_ticks_and_one_gated_batch_agree(rsa, O):
    sc, r, _, sched = _multi(O)
    n = sc.nd.n
    want = [_exp_after(r.exp[k], sched, n) for k in range(12)]
    missed = sum((w[1] for w in want), np.zeros(n, dtype=np.uint64))
    assert int(missed.sum()) >= 100
    tables = []
    for way in ("lone", "batch"):
        eng = _engine(rsa, sc.nd, sched, sc.params)
        try:
            if way == "lone":
                for k in range(12):
                    t0, tc, ts = sc.times(k)
                    eng.tick_run_sources_cca(t0, t0 + CR.TICK, r.lists[k], ts, CR.AIR, tc, sc.threshold)
                    _check_links(eng.result_copy(len(r.lists[k]), cap=1 << 22), r.exp[k], want[k][0], "gated tick %d" % k)
            else:
                got = _gated_batch(eng, sc, r.lists[:12], 0, "device", sc.threshold)
                for k in range(12):
                    np.testing.assert_array_equal(got[k][0], r.flags[k], err_msg="flags, tick %d" % k)   # the gate ignores schedules
                    np.testing.assert_array_equal(_bits(got[k][1]), _bits(r.energy[k]), err_msg="energy, tick %d" % k)
                    _check_links(eng.batch_result_copy(k, len(r.lists[k]), cap=1 << 22), r.exp[k], want[k][0], "gated batch, tick %d" % k)
            tables.append(eng.listen_missed())
            np.testing.assert_array_equal(tables[-1], missed, err_msg=way)
        finally:
            eng.close()
    np.testing.assert_array_equal(tables[0], tables[1])


def test_csma_whole_and_split_agree(rsa, O):
    """E8 as one batch and E9 as two carry batches cut in the middle: every (src, start, dst) has one verdict whatever the split
    (packet numbers differ: csma_carry_ref.live maps them), and the missed tables are equal"""
    sc, _, r, sched = _multi(O)
    n, (n_ticks, p) = sc.nd.n, SR.SCENES["multi"]
    t_cca = [sc.times(k)[1] for k in range(n_ticks)]
    missed = sum((_exp_after(r.exp[k], sched, n)[1] for k in range(n_ticks)), np.zeros(n, dtype=np.uint64))
    assert int(missed.sum()) >= 100
    seen, tables = [], []
    for cuts in ((), (6,)):
        eng, verdicts = _engine(rsa, sc.nd, sched, sc.params), {}
        try:
            edges, carry = [0] + list(cuts) + [n_ticks], None
            for first, last in zip(edges[:-1], edges[1:]):
                want_carry, ids = KR.carry_at(r, first, t_cca)
                carry = want_carry[:0] if carry is None else carry
                np.testing.assert_array_equal(carry, want_carry)   # the gate and the carry ignore schedules
                _, _, n_exp, carry = _part(rsa, eng, sc, r.lists[first:last], first, "device", sc.threshold, p, carry)
                alive = KR.live(r, first, last, ids)
                for b in range(last - first):
                    exp = KR.expected_links(r.exp[first + b], alive[b])
                    v, _, by_link = _exp_after(exp, sched, n)
                    _check_links(eng.batch_result_copy(b, int(n_exp[b]), cap=1 << 22), exp, v, "cuts %s, tick %d" % (cuts, first + b))
                    verdicts.update(by_link)
            tables.append(eng.listen_missed())
            np.testing.assert_array_equal(tables[-1], missed, err_msg="cuts %s" % (cuts,))
        finally:
            eng.close()
        seen.append(verdicts)
    assert seen[0] == seen[1] and len(seen[0]) > 1000
    np.testing.assert_array_equal(tables[0], tables[1])
    # ... and the whole as ONE CSMA-CA batch (E8's own entry point)
    eng = _engine(rsa, sc.nd, sched, sc.params)
    try:
        _, n_exp = _csma(rsa, eng, sc, r.lists, 0, "device", sc.threshold, p)
        one, alive = {}, KR.live(r, 0, n_ticks, KR.carry_at(r, 0, t_cca)[1])
        for b in range(n_ticks):
            exp = KR.expected_links(r.exp[b], alive[b])
            v, _, by_link = _exp_after(exp, sched, n)
            _check_links(eng.batch_result_copy(b, int(n_exp[b]), cap=1 << 22), exp, v, "one CSMA-CA batch, tick %d" % b)
            one.update(by_link)
        assert one == seen[0]
        np.testing.assert_array_equal(eng.listen_missed(), missed)
    finally:
        eng.close()


# ---- 6. the unicast query sees the verdict after the pass ----------------------------------------------------------------------

def test_unicast_query_sees_a_sleeping_destination(rsa, O):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("lone")
    run, srcs = runs[None], lists[0]
    fl = np.flatnonzero((run.before[0] == O.DELIVERED) & (run.after[0] != O.DELIVERED))
    q_of = {}
    for i in fl:   # one flipped link per packet
        q_of.setdefault(int(run.res[0].pkt[i]), int(run.res[0].dst[i]))
    want = np.full(len(srcs), -1, dtype=np.int32)
    for q, j in q_of.items():
        want[q] = j
    asked = want >= 0
    assert asked.sum() >= 20
    eng, d = _engine(rsa, nd, sched), DeviceArray(srcs)
    try:
        _lone(eng, "sources", d, srcs, starts[0], air)
        got = eng.unicast_query([want], fields=("status", "reply_src"))
        assert (got["status"][asked] == UC_INTERFERED).all() and (got["reply_src"] == -1).all()
        # the same packets with those nodes' periods set to 0
        idx = want[asked]
        eng.listen_set(np.zeros(len(idx), dtype=LR.DTYPE), idx)
        far = 100 * TICK
        _lone(eng, "sources", d, srcs, far, air, t0=far)
        got = eng.unicast_query([want], fields=("status", "reply_src"))
        assert (got["status"][asked] == UC_DELIVERED).all()
        np.testing.assert_array_equal(got["reply_src"][asked], idx)
    finally:
        d.free()
        eng.close()


# ---- 7. the dense medium ---------------------------------------------------------------------------------------------------------

def test_null_medium_ends_with_its_records(rsa, O):
    scene = S.scene_null()
    nd, kind, params, pk, _, _ = scene
    cpu = S.oracle_tick(scene)
    sched, _ = LR.schedule(nd.n, LR.SCHED_SEED, LR.reached_receivers([(cpu, cpu.verdict)]))
    after, missed = LR.apply(pk, cpu, sched)
    assert 1000 <= int(missed.sum()) <= cpu.count - 1000
    srcs = np.ascontiguousarray(pk["src"], dtype=np.int32)
    eng, d = rsa.Engine(0), DeviceArray(srcs)
    try:
        configure_engine(eng, nd, kind, params)
        eng.set_link_capacity(1 << 20)
        eng.listen_set(sched)
        eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, S.AIR)
        _refused(rsa, eng, STATE, eng.result_dense)
        got = eng.result_copy(len(srcs), cap=1 << 20)
        np.testing.assert_array_equal(got.dst, cpu.dst)
        np.testing.assert_array_equal(got.verdict, after)
        np.testing.assert_array_equal(eng.listen_missed(), missed)
        eng.listen_clear()
        eng.tick_run_sources_device(10 * TICK, 11 * TICK, d.ptr.value, len(srcs), 10 * TICK, S.AIR)
        if os.environ.get("RM_DENSE_TICK") != "0":   # (a run whose knobs never take the dense form has no masks to ask for)
            r = eng.result_dense()
            assert r.n_packets == len(srcs)
        off = eng.result_copy(len(srcs), cap=1 << 20)
        np.testing.assert_array_equal(off.dst, cpu.dst)
        np.testing.assert_array_equal(off.verdict, cpu.verdict)
    finally:
        d.free()
        eng.close()


# ---- 8. the reception stage --------------------------------------------------------------------------------------------------------

def test_reception_stage_loses_exactly_the_missed_pairs(rsa, O):
    nd, rng = R.nodes(1500, seed=8)
    lists = [np.sort(rng.choice(nd.n, 40, replace=False)).astype(np.int32) for _ in range(3)]
    starts = [0, TICK, 2 * TICK]
    plain = LR.Run(nd, lists, starts, 640, np.zeros(nd.n, dtype=LR.DTYPE))
    sched, _ = LR.schedule(nd.n, LR.SCHED_SEED, LR.reached_receivers(zip(plain.res, plain.before)))
    run = LR.Run(nd, lists, starts, 640, sched)
    lost, base = set(), 0
    for k, (w, before, after) in enumerate(zip(run.res, run.before, run.after)):
        for i in np.flatnonzero(before != after):
            lost.add((base + int(w.pkt[i]), int(w.dst[i])))
        base += len(lists[k])
    assert len(lost) >= 300
    got = []
    for s in (None, sched):
        eng, dev = _engine(rsa, nd, s), []
        try:
            eng.set_time(0)
            eng.events_enable()
            _run_batch(eng, lists, starts, 640, dev)
            got.append(eng.events_process_batch([TICK, 2 * TICK, 3 * TICK]))
            if s is not None:
                np.testing.assert_array_equal(eng.listen_missed(), run.missed)
        finally:
            for d in dev:
                d.free()
            eng.close()
    gone = 0
    for off, on in zip(*got):
        keep = np.array([(int(q), int(j)) not in lost for q, j in zip(off[0], off[1])], dtype=bool)
        np.testing.assert_array_equal(on[0], off[0][keep])
        np.testing.assert_array_equal(on[1], off[1][keep])
        np.testing.assert_array_equal(_bits(on[2]), _bits(off[2][keep]))
        gone += int((~keep).sum())
    assert gone == len(lost)


# ---- 9. large times, periods on both sides of 2^32 ------------------------------------------------------------------------------------

def test_large_times_and_long_periods(rsa, O):
    nd, lists, _, air, _, _, _, _ = LR.scene("lone")
    srcs, t0 = lists[0], 3 * 10 ** 12
    rng = np.random.default_rng(9)
    sched = np.zeros(nd.n, dtype=LR.DTYPE)
    sched["period_us"] = rng.choice(np.array([0, 3000, 125000, (1 << 31) + 3, (1 << 32) - 5, (1 << 32) + 7, 10 ** 10, 7 * 10 ** 12], dtype=np.int64), nd.n)
    sched["on_us"] = (sched["period_us"] * rng.uniform(0.2, 0.8, nd.n)).astype(np.int64)
    sched["phase_us"] = rng.integers(0, np.maximum(sched["period_us"], 1))
    run = LR.Run(nd, [srcs], [t0], air, sched)
    hit = sched["period_us"][run.res[0].dst[run.before[0] == O.DELIVERED]]
    for lo, hi in ((1, 1 << 32), (1 << 32, 1 << 62)):   # delivered links at receivers on both sides, flipped and kept
        assert ((hit >= lo) & (hit < hi)).sum() >= 500
    assert 500 <= int(run.missed.sum()) <= len(hit) - 500
    eng, d = _engine(rsa, nd, sched), DeviceArray(srcs)
    try:
        got = _lone(eng, "sources", d, srcs, t0, air, t0=t0)
        np.testing.assert_array_equal(got.dst, run.res[0].dst)
        np.testing.assert_array_equal(got.verdict, run.after[0])
        np.testing.assert_array_equal(eng.listen_missed(), run.missed)
    finally:
        d.free()
        eng.close()


# ---- 10. list updates and the tables' lifetime ----------------------------------------------------------------------------------------

def test_list_updates_and_lifetime(rsa, O):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("lone")
    srcs, w = lists[0], runs[None].res[0]
    eng, d = _engine(rsa, nd), DeviceArray(srcs)
    far, clock = 100 * TICK, [0]

    def tick(table):
        """a lone tick at the next far time -> the engine's verdicts and the reference's under `table` at that time"""
        t = clock[0]
        clock[0] += far
        got = _lone(eng, "sources", d, srcs, t, air, t0=t)
        new = LR.packets(nd, srcs, t, air)
        after, m = LR.apply(new, w, table, runs[None].before[0])
        np.testing.assert_array_equal(got.dst, w.dst)
        np.testing.assert_array_equal(got.verdict, after)
        return m

    try:
        for call in (eng.listen_get, eng.listen_missed, eng.listen_missed_reset, eng.listen_device):   # before the first set
            _refused(rsa, eng, STATE, call)
        eng.listen_set(sched)
        np.testing.assert_array_equal(eng.listen_get(), sched)
        total = tick(sched)
        # a list changes only the listed nodes; of a node named twice the last entry wins
        idx = np.array([7, int(w.dst[0]), 7, nd.n - 1, int(w.dst[5])], dtype=np.int32)
        recs = np.array([(1500, 0, 3), (2000, 0, 0), (3000, 3000, 2999), (0, 0, 0), (1, 0, 0)], dtype=LR.DTYPE)
        eng.listen_set(recs, idx)
        cur = sched.copy()
        for j, r in zip(idx, recs):
            cur[j] = r
        assert cur[7].tolist() == (3000, 3000, 2999)
        np.testing.assert_array_equal(eng.listen_get(), cur)
        np.testing.assert_array_equal(eng.listen_get(idx), cur[idx])
        p_s, p_m = eng.listen_device()
        np.testing.assert_array_equal(DeviceArray.read(p_s, rsa.LISTEN_SCHEDULE_DTYPE, nd.n), cur)
        total = total + tick(cur)
        np.testing.assert_array_equal(eng.listen_missed(), total)
        np.testing.assert_array_equal(DeviceArray.read(p_m, np.uint64, nd.n), total)
        big = np.random.default_rng(1).integers(0, nd.n, 5000).astype(np.int32)
        np.testing.assert_array_equal(eng.listen_missed(big), total[big])
        # a long list with many duplicates
        recs = LR.schedule(5000, 11)[0]
        eng.listen_set(recs, big)
        for j, r in zip(big, recs):
            cur[j] = r
        np.testing.assert_array_equal(DeviceArray.read(p_s, rsa.LISTEN_SCHEDULE_DTYPE, nd.n), cur)
        total = total + tick(cur)
        # the medium and the nodes may change: both tables stay
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
        eng.seed(3)
        i = int(srcs[0])
        eng.update_node(i, float(nd.x[i]), float(nd.y[i]), float(nd.z[i]), float(nd.txpower[i]), int(nd.channel[i]), 1, 1.0, 1.0)
        eng.upload_table(nd)
        assert eng.listen_enabled()
        np.testing.assert_array_equal(eng.listen_get(), cur)
        np.testing.assert_array_equal(eng.listen_missed(), total)
        total = total + tick(cur)
        np.testing.assert_array_equal(eng.listen_missed(), total)
        eng.listen_missed_reset()
        assert not eng.listen_missed().any()
        m = tick(cur)
        np.testing.assert_array_equal(eng.listen_missed(), m)
        # another node count clears the feature
        half = O.NodeTable(nd.n // 2)
        half.x, half.y = nd.x[:nd.n // 2], nd.y[:nd.n // 2]
        eng.upload_table(half)
        assert not eng.listen_enabled()
        _refused(rsa, eng, STATE, eng.listen_get)
        eng.listen_set(np.zeros(nd.n // 2, dtype=LR.DTYPE))
        assert eng.listen_enabled() and not eng.listen_missed().any() and not eng.listen_get()["period_us"].any()
    finally:
        d.free()
        eng.close()


def test_list_set_followed_at_once_by_a_list_read(rsa, O):
    """the list update and the list read stage through one host-mapped block: a read of other nodes directly behind an update must
    not reach the update's scatter -- the device's schedule table equals the host's copy after every pair, and the counts are right"""
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("lone")
    eng, d = _engine(rsa, nd, sched), DeviceArray(lists[0])
    try:
        _lone(eng, "sources", d, lists[0], starts[0], air)
        missed = runs[None].missed
        p_s, _ = eng.listen_device()
        cur, rng = sched.copy(), np.random.default_rng(4)
        for k, size in enumerate([1, 3, 64, 700, 5000, 2, 1]):
            a = rng.integers(0, nd.n, size).astype(np.int32)
            b = ((a + 1 + rng.integers(0, nd.n - 1, size)) % nd.n).astype(np.int32)   # other nodes than a, entry by entry
            recs = LR.schedule(size, 100 + k)[0]
            eng.listen_set(recs, a)
            got = eng.listen_missed(b)
            for j, r in zip(a, recs):
                cur[j] = r
            np.testing.assert_array_equal(got, missed[b], err_msg="read %d" % k)
            np.testing.assert_array_equal(DeviceArray.read(p_s, rsa.LISTEN_SCHEDULE_DTYPE, nd.n), cur, err_msg="table after pair %d" % k)
            np.testing.assert_array_equal(eng.listen_get(), cur)
    finally:
        d.free()
        eng.close()


# ---- 11. a slot over its link capacity --------------------------------------------------------------------------------------------------

def test_a_slot_over_the_link_capacity_counts_nothing(rsa, O):
    """test_gpu_stats' batch: a tick of 150 frames one link over the capacity and two small ticks that survive"""
    nd, lists, starts, air, sched, _, _, _ = LR.scene("batch")
    lists, starts = [lists[3], lists[4][:3], lists[5][:2]], starts[3:]
    run = LR.Run(nd, lists, starts, air, sched)
    cap = run.res[0].count - 1
    assert cap > 16384 and all(0 < 16 * w.count < cap for w in run.res[1:])
    missed = np.zeros(nd.n, dtype=np.uint64)
    for k in (1, 2):
        missed += LR.apply(run.new[k], run.res[k], sched, run.before[k])[1]
    assert missed.any() and int(run.missed.sum()) > int(missed.sum()) + 100
    eng, dev = _engine(rsa, nd, sched, cap=cap), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        assert [bool(eng.batch_result_count(k)[1]) for k in range(3)] == [True, False, False]
        np.testing.assert_array_equal(eng.listen_missed(), missed)
        for k in (1, 2):
            np.testing.assert_array_equal(eng.batch_result_copy(k, len(lists[k]), cap=1 << 20).verdict, run.after[k])
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 12. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_everything_as_it_was(rsa, O):
    from radio_sim_amd import _lib
    nd, lists, starts, air, sched, _, runs, _ = LR.scene("lone")
    srcs, w, before = lists[0], runs[None].res[0], runs[None].before[0]
    eng, d = _engine(rsa, nd, sched), DeviceArray(srcs)
    clock = [0]
    try:
        def plain(what):
            """a plain lone tick is the reference's (the window is unharmed) and adds exactly its own missed counts"""
            t = clock[0]
            clock[0] += 100 * TICK
            was = eng.listen_missed()
            got = _lone(eng, "sources", d, srcs, t, air, t0=t)
            after, m = LR.apply(LR.packets(nd, srcs, t, air), w, sched, before)
            np.testing.assert_array_equal(got.dst, w.dst, err_msg=what)
            np.testing.assert_array_equal(got.verdict, after, err_msg=what)
            np.testing.assert_array_equal(_bits(got.sinr), _bits(w.sinr), err_msg=what)
            np.testing.assert_array_equal(eng.listen_missed() - was, m, err_msg=what)

        def refused(what, call, partition=None, code=STATE):
            t = clock[0]
            was = (eng.listen_missed(), eng.listen_get(), eng.rng_state)
            if partition:
                partition()
            _refused(rsa, eng, code, lambda: call(t))
            if partition:
                eng.set_partition(0, nd.n)
            np.testing.assert_array_equal(eng.listen_missed(), was[0], err_msg=what)
            np.testing.assert_array_equal(eng.listen_get(), was[1], err_msg=what)
            assert eng.rng_state == was[2] and eng.listen_enabled(), what
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
        # every RM_ERR_INVALID of the spec: the whole list is validated before anything changes
        ok = np.array([(1000, 10, 0)], dtype=LR.DTYPE)
        for bad in [(0, 1, 0), (0, 0, 1), (-5, 0, 0), (1000, -1, 0), (1000, 1001, 0), (1000, 10, -1), (1000, 10, 1000)]:
            both = np.array([(1000, 10, 0), bad], dtype=LR.DTYPE)
            refused("a bad record %s" % (bad,), lambda t, both=both: eng.listen_set(both, np.array([3, 4], dtype=np.int32)), code=INVALID)
        whole = sched.copy()
        whole[nd.n - 1] = (0, 5, 0)
        refused("a bad record in a whole table", lambda t: eng.listen_set(whole), code=INVALID)
        for idx in ([0, nd.n], [-1, 0]):
            two = np.array([(1000, 10, 0), (1000, 10, 0)], dtype=LR.DTYPE)
            refused("index %s" % idx, lambda t, idx=idx: eng.listen_set(two, np.array(idx, dtype=np.int32)), code=INVALID)
            refused("get %s" % idx, lambda t, idx=idx: eng.listen_get(np.array(idx, dtype=np.int32)), code=INVALID)
            refused("missed %s" % idx, lambda t, idx=idx: eng.listen_missed(np.array(idx, dtype=np.int32)), code=INVALID)
        refused("no list, another count", lambda t: eng.listen_set(sched[:-1]), code=INVALID)
        L = _lib.lib()
        one = _lib.ListenSchedule(1000, 10, 0)
        out = np.zeros(nd.n, dtype=np.uint64)
        assert L.rm_listen_set(eng._h, None, nd.n, None) == INVALID and L.rm_listen_set(None, None, 0, None) == INVALID
        assert L.rm_listen_set(eng._h, None, -1, C.byref(one)) == INVALID
        assert L.rm_listen_get(eng._h, None, nd.n, None) == INVALID and L.rm_listen_get(eng._h, None, nd.n - 1, out.ctypes.data) == INVALID
        assert L.rm_listen_missed_read(eng._h, None, nd.n, None) == INVALID and L.rm_listen_missed_read(eng._h, None, -1, out.ctypes.data) == INVALID
        assert L.rm_listen_clear(None) == INVALID and L.rm_listen_missed_reset(None) == INVALID and L.rm_listen_device(None, None, None) == INVALID
        assert L.rm_listen_enabled(None) == 0
        np.testing.assert_array_equal(eng.listen_get(), sched)
        plain("after the invalid calls")
        # a reference medium too (its ticks take other entry points)
        eng.set_model(1)
        eng.set_partition(0, nd.n // 2)
        _refused(rsa, eng, STATE, lambda: flush(clock[0]))
        _refused(rsa, eng, STATE, lambda: eng.tick_run_sources_device(clock[0], clock[0] + TICK, d.ptr.value, len(srcs), clock[0], air))
        _refused(rsa, eng, STATE, lambda: eng.transmit(int(srcs[0]), clock[0], 254, cap=1 << 16))
        eng.set_partition(0, nd.n)
        # rm_group_*: a member with schedules refuses the group's tick (a group of one too); cleared, the group's tick runs
        grp = rsa.Group([0])
        try:
            grp.upload_table(nd)
            grp.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
            member = L.rm_group_context(grp._h, 0)
            tbl = np.ascontiguousarray(sched)
            assert L.rm_listen_set(member, None, nd.n, tbl.ctypes.data) == 0 and L.rm_listen_enabled(member) == 1
            recs = to_tx_records(rsa, nd.packets(srcs, 0, air))
            _refused(rsa, grp, STATE, lambda: grp.tick(recs, 0, TICK, cap=1 << 20))
            assert L.rm_listen_missed_read(member, None, nd.n, out.ctypes.data) == 0 and not out.any()
            assert L.rm_listen_clear(member) == 0 and L.rm_listen_enabled(member) == 0
            got = grp.tick(recs, 0, TICK, cap=1 << 20)
            assert got.count == w.count
            np.testing.assert_array_equal(got.verdict, before)
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
        eng.listen_set(np.zeros((4, 3), dtype=np.int64))
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        assert not eng.listen_enabled()
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_set_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs: the pass is not part of them"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)
