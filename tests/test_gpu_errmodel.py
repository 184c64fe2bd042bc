"""The frame error model of the SINR medium (rm_set_error_model, rm_errmodel.hip) on the GPU.  Expected
values come from the oracle plus tests/errmodel_ref.py alone (tests/test_errmodel_ref.py holds the scenes' conditions for that
reference).  Every comparison is bit for bit on (dst, verdict, rssi bits, sinr bits, pkt_offset, pkt_interference)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import cca_batch_ref as BR
import cca_ref as CR
import csma_carry_ref as KR
import csma_ref as SR
import errmodel_ref as R
from test_gpu_cca import _bits, _engine as _plain_engine
from test_gpu_cca_batch import _batch, _refused, _times
from test_gpu_csma_carry import _part, _same_table
from util import DeviceArray

pytestmark = pytest.mark.gpu

TICK = R.TICK
NAN = float("nan")
EM_KERNELS = ("k_errmodel", "k_errmodel_batch")


def _engine(rsa, nd, params=R.PARAMS, seed=R.SEED, cap=None):
    eng = _plain_engine(rsa, nd, params, cap)
    if seed is not None:
        eng.set_error_model(rsa.EM_OQPSK_250K, seed=seed)
    return eng


def _same(gpu, want, what, verdict=None):
    assert gpu.count == want.count, (what, gpu.count, want.count)
    np.testing.assert_array_equal(gpu.pkt, want.pkt, err_msg=what + ": pkt")
    np.testing.assert_array_equal(gpu.dst, want.dst, err_msg=what + ": dst")
    np.testing.assert_array_equal(gpu.verdict, want.verdict if verdict is None else verdict, err_msg=what + ": verdict")
    np.testing.assert_array_equal(_bits(gpu.rssi), _bits(want.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(gpu.sinr), _bits(want.sinr), err_msg=what + ": sinr")
    np.testing.assert_array_equal(gpu.pkt_offset, want.pkt_offset, err_msg=what + ": pkt_offset")
    np.testing.assert_array_equal(gpu.pkt_interference[want.slots], want.pkt_interference[want.slots], err_msg=what + ": Tx-failure flags")


def test_lone_ticks_of_every_form(rsa, O):
    """one tick of 60 frames through rm_tick_flush, rm_tick_flush_view and rm_tick_run_sources_device + rm_result_copy"""
    nd, srcs, start, air = R.scene_lone()
    want, _ = R.Replay(nd).tick(0, srcs, start, air)
    assert (want.verdict != want.plain).sum() >= 50
    d = DeviceArray(srcs)
    try:
        for form in ("flush", "view", "sources"):
            eng = _engine(rsa, nd)
            try:
                if form == "sources":
                    eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), start, air)
                    got = eng.result_copy(len(srcs), cap=1 << 20)
                else:
                    eng.tick_begin(0, TICK)
                    for s in srcs:
                        eng.enqueue_tx(int(s), start, air)
                    got = eng.tick_flush(cap=1 << 20) if form == "flush" else eng.tick_flush_view()
                _same(got, want, form)
            finally:
                eng.close()
    finally:
        d.free()


def test_transmit_packet_by_packet_equals_one_tick(rsa, O):
    """30 frames that do not overlap: rm_transmit one by one and one rm_tick_flush over all of them"""
    nd, srcs, starts, hex_len, air = R.scene_serial()
    rep = R.Replay(nd)
    wants = [rep.tick(int(s), [q], int(s), air)[0] for q, s in zip(srcs, starts)]
    a, b = _engine(rsa, nd), _engine(rsa, nd)
    try:
        for k, (q, s) in enumerate(zip(srcs, starts)):
            got = a.transmit(int(q), int(s), hex_len, cap=1 << 16)
            _same(got, wants[k], "rm_transmit %d" % k)
        b.tick_begin(0, int(starts[-1]) + air)
        for q, s in zip(srcs, starts):
            b.enqueue_tx(int(q), int(s), air)
        got = b.tick_flush(cap=1 << 20)
        np.testing.assert_array_equal(got.dst, np.concatenate([w.dst for w in wants]))
        np.testing.assert_array_equal(got.verdict, np.concatenate([w.verdict for w in wants]))
        np.testing.assert_array_equal(_bits(got.sinr), _bits(np.concatenate([w.sinr for w in wants])))
        np.testing.assert_array_equal(got.pkt_offset, np.concatenate([[0], np.cumsum([w.count for w in wants])]))
    finally:
        a.close()
        b.close()


def _run_batch(eng, lists, starts, air, dev):
    arrs = [DeviceArray(s) if len(s) else None for s in lists]
    dev.extend(a for a in arrs if a is not None)
    eng.batch_run_sources_device(starts, [s + TICK for s in starts], [a.ptr.value if a is not None else 0 for a in arrs],
                                 [len(s) for s in lists], starts, [air] * len(lists))


@pytest.mark.parametrize("overlap", [False, True])
def test_batches_of_both_kinds(rsa, O, overlap):
    """six ticks (an empty list, padding entries, link counts that are no multiple of 64, one slot above 16 384 links) as one batch of
    self-contained ticks / of ticks whose frames outlive them, read through rm_batch_result_copy and rm_batch_result_view; the model
    switched off again gives the plain oracle"""
    nd, lists, starts, air = R.scene_batch(overlap)
    rep = R.Replay(nd)
    wants = [rep.tick(s, l, s, air)[0] for l, s in zip(lists, starts)]
    assert max(w.count for w in wants) > 16384 and wants[1].count == 0
    eng, dev = _engine(rsa, nd), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        assert eng.air_batch_stats()[0] == (1 if overlap else 0)
        for b, w in enumerate(wants):
            _same(eng.batch_result_copy(b, len(lists[b]), cap=1 << 20), w, "copy, tick %d" % b)
        views, status = eng.batch_result_view(len(lists))
        assert status == [0] * len(lists)
        for b, w in enumerate(wants):
            _same(views[b], w, "view, tick %d" % b)
        # off again: the same ticks later in time are the plain oracle's
        eng.set_error_model(rsa.EM_NONE)
        assert eng.get_error_model().kind == rsa.EM_NONE
        later = [s + 100 * TICK for s in starts]
        _run_batch(eng, lists, later, air, dev)
        for b, (l, s) in enumerate(zip(lists, later)):
            w, _ = rep.tick(s, l, s, air)
            _same(eng.batch_result_copy(b, len(l), cap=1 << 20), w, "model off, tick %d" % b, verdict=w.plain)
    finally:
        for d in dev:
            d.free()
        eng.close()


def _e10_scene(O):
    """cca_ref's scene "multi" with the curve's parameters: sensing reads neither the sensitivity nor the capture threshold"""
    sc = copy.copy(BR.scene(O, "multi"))
    sc.params = dict(sc.params, ld_noise_dbm=-100.0, ld_sensitivity_dbm=-103.0, ld_capture_db=R.NINF)
    return sc


_E10_CACHE = {}


def _e10_links(exp):
    """a tick's cca_ref.Expected with E10 applied to its verdict column"""
    if exp.raw is None:
        return np.zeros(0, dtype=np.uint8), {}
    if id(exp.raw) not in _E10_CACHE:   # (a split's parts share the whole run's oracle results)
        _E10_CACHE[id(exp.raw)] = (exp.raw, R.apply_full(exp.new, exp.raw, R.SEED)[0])
    v = _E10_CACHE[id(exp.raw)][1]
    pk = exp.new[exp.raw.pkt]
    return v, {(int(s), int(t), int(d)): int(x) for s, t, d, x in zip(pk["src"], pk["start_us"], exp.raw.dst, v)}


def _same_exp(gpu, exp, verdict, what):
    assert gpu.count == exp.count, (what, gpu.count, exp.count)
    np.testing.assert_array_equal(gpu.pkt, exp.pkt, err_msg=what + ": pkt")
    np.testing.assert_array_equal(gpu.dst, exp.dst, err_msg=what + ": dst")
    np.testing.assert_array_equal(gpu.verdict, verdict, err_msg=what + ": verdict")
    np.testing.assert_array_equal(_bits(gpu.rssi), _bits(exp.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(gpu.sinr), _bits(exp.sinr), err_msg=what + ": sinr")
    np.testing.assert_array_equal(gpu.pkt_offset, exp.pkt_offset, err_msg=what + ": pkt_offset")
    np.testing.assert_array_equal(gpu.pkt_interference[exp.slots], exp.pkt_interference, err_msg=what + ": Tx-failure flags")


def test_gated_batch_with_the_model_on(rsa, O):
    """E7: flags and energies as cca_batch_ref gives them, the links with E10 applied"""
    sc = _e10_scene(O)
    r = BR.Run(O, sc, 8)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        got = _batch(eng, sc, r.lists, 0, "device", sc.threshold)
        flipped = 0
        for k in range(8):
            np.testing.assert_array_equal(got[k][0], r.flags[k], err_msg="flags, tick %d" % k)
            np.testing.assert_array_equal(_bits(got[k][1]), _bits(r.energy[k]), err_msg="energy, tick %d" % k)
            v, _ = _e10_links(r.exp[k])
            flipped += int((v != r.exp[k].verdict).sum())
            _same_exp(eng.batch_result_copy(k, len(r.lists[k]), cap=1 << 22), r.exp[k], v, "gated tick %d" % k)
        assert flipped >= 50
    finally:
        eng.close()


def test_csma_batch_whole_and_split_give_the_same_verdicts(rsa, O):
    """E8 as one batch and E9 as two carry batches: the gate's tables equal csma_ref / csma_carry_ref as without the model, the links
    equal the reference with E10 applied, and every (src, start, dst) has one verdict whatever the split -- packet numbers differ"""
    sc = _e10_scene(O)
    n_ticks, p = SR.SCENES["multi"]
    r = SR.Run(O, sc, sc.ticks[:n_ticks], p)
    t_cca = [sc.times(k)[1] for k in range(n_ticks)]
    seen = []
    for cuts in ((), (6,)):
        eng = _engine(rsa, sc.nd, sc.params)
        verdicts, flipped = {}, 0
        try:
            edges, carry = [0] + list(cuts) + [n_ticks], None
            for first, last in zip(edges[:-1], edges[1:]):
                what = "cuts %s, ticks %d .. %d" % (cuts, first, last - 1)
                want_carry, ids = KR.carry_at(r, first, t_cca)
                carry = want_carry[:0] if carry is None else carry
                np.testing.assert_array_equal(carry, want_carry, err_msg=what + ": carry-in")
                out, carried, n_exp, carry = _part(rsa, eng, sc, r.lists[first:last], first, "device", sc.threshold, p, carry)
                alive = KR.live(r, first, last, ids)
                np.testing.assert_array_equal(n_exp, [len(a) for a in alive], err_msg=what + ": n_exp")
                own_w, car_w = KR.tables_of(r, first, last, ids, want_carry)
                _same_table(out, own_w, what + ", own table")
                _same_table(carried, car_w, what + ", carried table")
                for b in range(last - first):
                    exp = KR.expected_links(r.exp[first + b], alive[b])
                    v, by_link = _e10_links(exp)
                    flipped += int((v != exp.verdict).sum())
                    _same_exp(eng.batch_result_copy(b, int(n_exp[b]), cap=1 << 22), exp, v, "%s, tick %d" % (what, first + b))
                    verdicts.update(by_link)
        finally:
            eng.close()
        assert flipped >= 50
        seen.append(verdicts)
    assert seen[0] == seen[1] and len(seen[0]) > 1000


def test_reception_stage_gets_the_new_verdicts(rsa, O):
    """events on: three lone ticks, each drained, then a batch of three through rm_events_process_batch -- the deliveries are those of
    the oracle's Sim fed the E10 verdicts"""
    nd, rng = R.nodes(1500, seed=8)
    rep, sim = R.Replay(nd), O.Sim(nd.n)
    eng, dev = _engine(rsa, nd), []
    try:
        eng.set_time(0)
        eng.events_enable()
        lists = [np.sort(rng.choice(nd.n, 40, replace=False)).astype(np.int32) for _ in range(6)]
        base, delivered, withheld = 0, 0, 0

        def feed(k):
            nonlocal base, withheld
            w, _ = rep.tick(k * TICK, lists[k], k * TICK, 640)
            sim.medium_calls(w, nd.packets(lists[k], k * TICK, 640), pkt_base=base)
            base += len(lists[k])
            withheld += int((w.verdict != w.plain).sum())

        def check(got, t):
            nonlocal delivered
            ev = sim.step(t)
            ev = ev[ev["kind"] == O.EV_RX_END_DELIVERY]
            pkt, dst, rssi, _ = got
            np.testing.assert_array_equal(pkt, ev["pkt"])
            np.testing.assert_array_equal(dst, ev["node"])
            np.testing.assert_array_equal(_bits(rssi), _bits(ev["rssi"]))
            delivered += len(pkt)

        for k in range(3):
            d = DeviceArray(lists[k])
            dev.append(d)
            eng.tick_run_sources_device(k * TICK, (k + 1) * TICK, d.ptr.value, 40, k * TICK, 640)
            feed(k)
            check(eng.events_process((k + 1) * TICK), (k + 1) * TICK)
        _run_batch(eng, lists[3:], [3 * TICK, 4 * TICK, 5 * TICK], 640, dev)
        got = eng.events_process_batch([4 * TICK, 5 * TICK, 6 * TICK])
        for k in range(3, 6):
            feed(k)
            check(got[k - 3], (k + 1) * TICK)
        assert delivered > 1000 and withheld >= 50
    finally:
        for d in dev:
            d.free()
        eng.close()
        sim.close()


def test_shuffle_invariance(rsa, O):
    """the same frames in a permuted candidate order: one verdict per (src, start, dst)"""
    nd, srcs, start, air = R.scene_lone()
    rng = np.random.default_rng(4)
    seen = []
    for order in (srcs, rng.permutation(srcs)):
        eng, d = _engine(rsa, nd), DeviceArray(np.ascontiguousarray(order, dtype=np.int32))
        try:
            eng.tick_run_sources_device(0, TICK, d.ptr.value, len(order), start, air)
            got = eng.result_copy(len(order), cap=1 << 20)
            seen.append({(int(order[q]), int(x)): int(v) for q, x, v in zip(got.pkt, got.dst, got.verdict)})
        finally:
            d.free()
            eng.close()
    assert seen[0] == seen[1] and len(seen[0]) > 5000


def test_model_off_launches_nothing_and_on_launches_once_per_batch(rsa, O):
    nd, lists, starts, air = R.scene_batch(True)
    lists = [l for l in lists if len(l)]
    starts = starts[:len(lists)]
    rep = R.Replay(nd)
    for on in (False, True):
        eng, dev = _engine(rsa, nd, seed=R.SEED if on else None), []
        try:
            assert eng.get_error_model().kind == (rsa.EM_OQPSK_250K if on else rsa.EM_NONE)
            eng.profile_enable(1)
            _run_batch(eng, lists, starts, air, dev)
            if not on:   # a fresh context: the plain oracle
                for b, (l, s) in enumerate(zip(lists, starts)):
                    w, _ = rep.tick(s, l, s, air)
                    _same(eng.batch_result_copy(b, len(l), cap=1 << 20), w, "fresh context, tick %d" % b, verdict=w.plain)
            eng.sync()
            k = eng.profile_kernels()
            launches = {name: k[name][0] if isinstance(k[name], (tuple, list)) else k[name] for name in k if name in EM_KERNELS}
            assert launches == ({"k_errmodel_batch": 1} if on else {}), (launches, sorted(k))
            if on:
                _run_batch(eng, lists, [s + 50 * TICK for s in starts], air, dev)
                eng.sync()
                k = eng.profile_kernels()
                n = k["k_errmodel_batch"]
                assert (n[0] if isinstance(n, (tuple, list)) else n) == 2
        finally:
            for d in dev:
                d.free()
            eng.close()


def test_draws_come_first_then_the_pass(rsa, O):
    """rxProbability < 1 on an unpartitioned context: the java.util.Random draws decide first (the generator's state is the plain
    oracle's: the model consumes no draw), then E10 over what is still RM_DELIVERED"""
    from util import oracle_model
    nd, srcs, start, air = R.scene_lone()
    nd.rxprob[::3] = 0.5
    pk = nd.packets(srcs, start, air)
    res = O.tick(oracle_model(O, "logdist", R.PARAMS), nd, pk, rng_state=O.lib().orc_jrandom_seed(5), cap=1 << 22)
    assert res.pkt_draws.sum() > 100
    v, _ = R.apply_full(pk, res, R.SEED)
    assert (v != res.verdict).sum() >= 50
    eng, d = _engine(rsa, nd), DeviceArray(srcs)
    try:
        eng.seed(5)
        eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), start, air)
        got = eng.result_copy(len(srcs), cap=1 << 20)
        assert got.count == res.count
        np.testing.assert_array_equal(got.dst, res.dst)
        np.testing.assert_array_equal(_bits(got.sinr), _bits(res.sinr))
        np.testing.assert_array_equal(got.verdict, v)
        assert eng.rng_state == res.rng_state
    finally:
        d.free()
        eng.close()


def test_refusals_leave_the_context_unharmed(rsa, O):
    nd, srcs, start, air = R.scene_lone()
    want, _ = R.Replay(nd).tick(0, srcs, start, air)
    eng = _plain_engine(rsa, nd, R.PARAMS)
    d = DeviceArray(srcs)
    try:
        inval, state = -1, -5
        _refused(rsa, eng, inval, lambda: eng.set_error_model(7))
        _refused(rsa, eng, inval, lambda: eng.set_error_model(rsa.EM_OQPSK_250K, reserved=1))
        for upb in (0.0, -4.0, NAN, float("inf")):
            _refused(rsa, eng, inval, lambda: eng.set_error_model(rsa.EM_OQPSK_250K, us_per_bit=upb))
        assert eng.get_error_model().kind == rsa.EM_NONE
        # not the SINR medium
        eng.set_model(4, flags=0)
        _refused(rsa, eng, state, lambda: eng.set_error_model(rsa.EM_OQPSK_250K))
        eng.set_model(1)
        _refused(rsa, eng, state, lambda: eng.set_error_model(rsa.EM_OQPSK_250K))
        # rm_set_model switches the model off
        eng2 = _engine(rsa, nd)
        try:
            eng2.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
            assert eng2.get_error_model().kind == rsa.EM_NONE
        finally:
            eng2.close()
        # While a model is on: every refused evaluating call is followed by a plain lone tick (a later time each: the frames of the
        # call before have left the air) that is the reference's -- the context and its window are unharmed
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
        eng.set_error_model(rsa.EM_OQPSK_250K, seed=R.SEED)
        e = eng.get_error_model()
        assert (e.kind, e.us_per_bit, e.seed) == (rsa.EM_OQPSK_250K, 4.0, R.SEED)
        clock = [0]

        def plain(what):
            t = clock[0]
            clock[0] += 20 * TICK
            w, _ = R.Replay(nd).tick(t, srcs, t, air)
            eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air)
            _same(eng.result_copy(len(srcs), cap=1 << 20), w, "plain tick after " + what)

        def refused_on_partition(what, call):
            t = clock[0]
            eng.set_partition(0, nd.n // 2)
            _refused(rsa, eng, state, lambda: call(t))
            eng.set_partition(0, nd.n)
            plain(what)

        plain("setting the model")
        refused_on_partition("a lone tick on a partition", lambda t: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air))
        refused_on_partition("a batch on a partition",
                             lambda t: eng.batch_run_sources_device([t], [t + TICK], [d.ptr.value], [len(srcs)], [t], [air]))

        def flush(t):
            eng.tick_begin(t, t + TICK)
            eng.enqueue_tx(int(srcs[0]), t, air)
            eng.tick_flush(cap=1 << 16)
        refused_on_partition("rm_tick_flush on a partition", flush)   # (the refused tick is gone: the plain call starts its own)
        refused_on_partition("rm_transmit on a partition", lambda t: eng.transmit(int(srcs[0]), t, 254, cap=1 << 16))
        # the gathered and rm_dist_* forms, on the unpartitioned context (a world of one)
        for what, call in (
                ("gathered sources", lambda t: eng.batch_run_gathered_sources_device([t], [t + TICK], d.ptr.value, 1, len(srcs), [t], air)),
                ("rm_dist_batch", lambda t: eng.dist_batch_run_sources_device([t], [t + TICK], d.ptr.value, len(srcs), [t], air)),
                ("rm_dist_tick", lambda t: eng.dist_tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air))):
            t = clock[0]
            _refused(rsa, eng, state, lambda: call(t))
            plain(what)
        # rm_group_*: a member with a model refuses the group's tick; with the model off again the group's tick is the plain oracle's
        from radio_sim_amd import _lib
        grp = rsa.Group([0])
        try:
            grp.upload_table(nd)
            grp.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
            member = _lib.lib().rm_group_context(grp._h, 0)
            em = rsa.Engine.error_model(seed=R.SEED)
            assert _lib.lib().rm_set_error_model(member, C.byref(em)) == 0
            recs = np.zeros(len(srcs), dtype=rsa.TX_RECORD_DTYPE)
            pk = nd.packets(srcs, 0, air)
            for f in ("x", "y", "z", "txpower", "txprob", "start_us", "air_us", "src", "channel"):
                recs[f] = pk[f]
            _refused(rsa, grp, state, lambda: grp.tick(recs, 0, TICK, cap=1 << 20))
            em.kind = rsa.EM_NONE
            assert _lib.lib().rm_set_error_model(member, C.byref(em)) == 0
            _same(grp.tick(recs, 0, TICK, cap=1 << 20), want, "the group's tick, model off", verdict=want.plain)
        finally:
            grp.close()
        # a context made under RM_GRAPH=1 replays its ticks from captured graphs: the pass is not part of them
        os.environ["RM_GRAPH"] = "1"
        try:
            eng3 = _plain_engine(rsa, nd, R.PARAMS)
        finally:
            del os.environ["RM_GRAPH"]
        try:
            _refused(rsa, eng3, state, lambda: eng3.set_error_model(rsa.EM_OQPSK_250K))
            eng3.set_error_model(rsa.EM_NONE)
            eng3.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), start, air)
            _same(eng3.result_copy(len(srcs), cap=1 << 20), want, "RM_GRAPH=1, model off", verdict=want.plain)
        finally:
            eng3.close()
    finally:
        d.free()
        eng.close()
