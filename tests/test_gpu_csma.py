"""The CSMA-CA gated batch (rm_batch_run_sources_csma*) on the GPU.  Expected values come from the oracle alone
(tests/csma_ref.py: the schedule restated in Python, then tick by tick through cca_ref.Chain; tests/test_csma_ref.py holds the scenes'
conditions).  Everything is compared bit for bit: status, attempts, tick, pkt, flags and energy bits per packet; n_exp; per tick count,
pkt, dst, verdict, rssi, sinr, pkt_offset and the Tx-failure flags; the window after the batch through rm_channel_energy."""
import numpy as np
import pytest

import cca_batch_ref as BR
import cca_ref as CR
import csma_ref as SR
import energy_ref as R
from test_gpu_cca import _bits, _engine, _same_links, _same_sense
from test_gpu_cca_batch import _batch, _refused, _times
from util import DeviceArray

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = {"status": 77, "attempts": 78, "tick": -777, "pkt": -778, "flags": 79, "energy_dbm": 12345.0}


def _params(rsa, p, reserved=None):
    return rsa.Engine.csma_params(p.max_backoffs, p.min_be, p.max_be, p.seed, reserved)


def _csma(rsa, eng, sc, lists, first, form, thr, p, air=CR.AIR, fields=None, no_out=False):
    """ticks first .. of the scene's clock as ONE CSMA-CA gated batch -> ({field: per packet}, n_exp); the device form through device
    arrays (fields: the outputs asked for, the others stay NULL), with the caller's lists checked to be unwritten"""
    lists = [np.ascontiguousarray(s, dtype=np.int32) for s in lists]
    tb, te, tc, ts = _times(sc, first, first + len(lists))
    airs = list(air) if isinstance(air, (list, tuple)) else [air] * len(lists)
    names = [f for f, _ in rsa.Engine.CSMA_FIELDS] if fields is None else list(fields)
    if form == "host":
        return eng.batch_run_sources_csma(tb, te, lists, ts, airs, tc, thr, _params(rsa, p), fields=names)
    total = sum(len(s) for s in lists)
    d_s = [DeviceArray(s) if len(s) else None for s in lists]
    d_o = {f: DeviceArray(np.full(max(total, 1), SENTINEL[f], dtype=t)) for f, t in rsa.Engine.CSMA_FIELDS if f in names}
    try:
        n_exp = eng.batch_run_sources_csma_device(tb, te, [d.ptr.value if d else None for d in d_s], [len(s) for s in lists], ts, airs, tc, thr,
                                                  _params(rsa, p), None if no_out else {f: d.ptr.value for f, d in d_o.items()})
        eng.sync()
        for d, s in zip(d_s, lists):
            if d:
                np.testing.assert_array_equal(DeviceArray.read(d.ptr.value, np.int32, len(s)), s, err_msg="a caller's dev_src was written")
        types = dict(rsa.Engine.CSMA_FIELDS)
        return {f: DeviceArray.read(d.ptr.value, types[f], max(total, 1))[:total] for f, d in d_o.items()}, n_exp
    finally:
        for d in d_s + list(d_o.values()):
            if d:
                d.free()


def _same_packets(out, r, what):
    want = {"status": r.status, "attempts": r.attempts, "tick": r.tick, "pkt": r.pkt, "flags": r.flags}
    for f, w in want.items():
        if f in out:
            np.testing.assert_array_equal(out[f], w, err_msg="%s: %s" % (what, f))
    if "energy_dbm" in out:
        np.testing.assert_array_equal(_bits(out["energy_dbm"]), _bits(r.energy), err_msg=what + ": energy bits")


def _check(eng, r, out, n_exp, what):
    np.testing.assert_array_equal(n_exp, r.n_exp, err_msg=what + ": n_exp")
    _same_packets(out, r, what)
    for b in range(len(r.n_exp)):
        _same_links(eng.batch_result_copy(b, int(r.n_exp[b]), cap=1 << 22), r.exp[b], "%s, tick %d" % (what, b))


def _window_is(eng, O, sc, r, last_tick, what):
    """the frames on the air after the batch, through the query, the batch's nodes among the queried ones"""
    t = sc.times(last_tick)[2] + 1
    rng = np.random.default_rng(77)
    nodes = np.concatenate(r.lists[-8:] + [rng.integers(0, sc.nd.n, 100).astype(np.int32)])
    nodes = np.unique(nodes[(nodes >= 0) & (nodes < sc.nd.n)]).astype(np.int32)
    want = R.channel_energy(O, sc.model(O), sc.nd, r.onair[-1], t, nodes=nodes, threshold=-90.0)
    got = eng.channel_energy(t, nodes=nodes, cca_threshold_dbm=-90.0)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": window flags")
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=what + ": window energy")


def _kernels(eng):
    return {k for k in eng.profile_kernels() if k.startswith("k_csma") or k.startswith("k_ccab")}


GRID = {"k_ccab_begin", "k_csma_index<true>", "k_csma_pairs<true, false>", "k_ccab_scan_sums", "k_ccab_scan_top", "k_ccab_scan_offsets",
        "k_csma_pairs<true, true>", "k_csma_resolve"}


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name", ["multi", "ch16"])
def test_scene(rsa, O, name, form):
    """multi: 12 ticks x 150 candidates, parameters 4, 1, 3: packets sent at every attempt number, failed, pending, sibling losses.
    ch16: 11 ticks x 900 candidates on sixteen channels, expanded lists of up to 3624 slots: the resolve pass strides four times"""
    sc, r = BR.scene(O, name), SR.run(O, name)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        eng.profile_enable(1)
        out, n_exp = _csma(rsa, eng, sc, r.lists, 0, form, sc.threshold, SR.SCENES[name][1])
        _check(eng, r, out, n_exp, "%s, %s form" % (name, form))
        _window_is(eng, O, sc, r, len(r.lists) - 1, "%s, %s form" % (name, form))
        assert _kernels(eng) == GRID, _kernels(eng)
    finally:
        eng.close()


def test_e7_identity(rsa, O):
    """max_backoffs = 0: expanded lists equal the lists, flags / energy and every tick's results equal rm_batch_run_sources_cca's"""
    sc = BR.scene(O, "multi")
    lists = sc.ticks[:12]
    a, b = _engine(rsa, sc.nd, sc.params), _engine(rsa, sc.nd, sc.params)
    try:
        out, n_exp = _csma(rsa, a, sc, lists, 0, "device", sc.threshold, SR.Params(0, 1, 3, 7))
        e7 = _batch(b, sc, lists, 0, "device", sc.threshold)
        np.testing.assert_array_equal(n_exp, [len(s) for s in lists])
        _same_sense((out["flags"], out["energy_dbm"]), (np.concatenate([f for f, _ in e7]), np.concatenate([e for _, e in e7])), "E7 identity")
        real = np.concatenate(lists) >= 0
        assert set(out["status"][real].tolist()) == {SR.SENT, SR.FAILED} and not out["status"][~real].any()
        np.testing.assert_array_equal(out["status"][real] == SR.SENT, out["flags"][real] == 0)
        for k, src in enumerate(lists):
            ra, rb = a.batch_result_copy(k, len(src), cap=1 << 22), b.batch_result_copy(k, len(src), cap=1 << 22)
            assert ra.count == rb.count > 0
            for f in ("pkt", "dst", "verdict", "pkt_interference", "pkt_offset"):
                np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg="tick %d: %s" % (k, f))
            for f in ("rssi", "sinr"):
                np.testing.assert_array_equal(_bits(getattr(ra, f)), _bits(getattr(rb, f)), err_msg="tick %d: %s" % (k, f))
    finally:
        a.close()
        b.close()


def test_lone_tick_identity(rsa, O):
    """The reference's made-lists of multi, tick by tick as rm_tick_run_sources_cca_device on a second context, give the batch's flags
    and energy bits for every made slot that is not a sibling loser.  (A sibling loser's slot is padding in the list handed to the lone
    tick: the lone gate has no first-wins rule and would put a second frame of the node on the air.)"""
    sc, r = BR.scene(O, "multi"), SR.run(O, "multi")
    a, b = _engine(rsa, sc.nd, sc.params), _engine(rsa, sc.nd, sc.params)
    try:
        out, n_exp = _csma(rsa, a, sc, r.lists, 0, "device", sc.threshold, SR.SCENES["multi"][1])
        _same_packets(out, r, "multi")
        last_flags, last_energy = np.zeros(len(r.status), dtype=np.uint8), np.full(len(r.status), np.nan)
        compared = 0
        for T in range(len(r.lists)):
            t0, tc, ts = sc.times(T)
            loser = (r.made[T] >= 0) & (r.kept[T] < 0) & (r.slot_flags[T] == R.ED_TRANSMITTING) & _has_earlier_winner(r.made[T], r.kept[T])
            src = np.where(loser, -1, r.made[T]).astype(np.int32)
            d, d_f, d_e = DeviceArray(src), DeviceArray(np.zeros(len(src), dtype=np.uint8)), DeviceArray(np.zeros(len(src)))
            b.tick_run_sources_cca_device(t0, t0 + CR.TICK, d.ptr.value, len(src), ts, CR.AIR, tc, sc.threshold, d_f.ptr.value, d_e.ptr.value)
            b.sync()
            f, e = DeviceArray.read(d_f.ptr.value, np.uint8, len(src)), DeviceArray.read(d_e.ptr.value, np.float64, len(src))
            for x in (d, d_f, d_e):
                x.free()
            sel = src >= 0
            _same_sense((f[sel], e[sel]), (r.slot_flags[T][sel], r.slot_energy[T][sel]), "lone tick %d" % T)
            _same_links(b.result_copy(len(src), cap=1 << 22), r.exp[T], "lone tick %d" % T)
            for i in np.flatnonzero(sel):
                o = r.sched[T][i][0]
                last_flags[o], last_energy[o] = f[i], e[i]
            compared += int(sel.sum())
        # ... and the batch's per-packet outputs are those of the packets' last lone attempts (sibling losers aside)
        lost_last = np.zeros(len(r.status), dtype=bool)
        for T in range(len(r.lists)):
            for i, (o, a_, _) in enumerate(r.sched[T]):
                if r.made[T][i] >= 0:
                    lost_last[o] = r.kept[T][i] < 0 and r.slot_flags[T][i] == R.ED_TRANSMITTING and _has_earlier_winner(r.made[T], r.kept[T])[i]
        ok = (r.attempts > 0) & ~lost_last
        _same_sense((out["flags"][ok], out["energy_dbm"][ok]), (last_flags[ok], last_energy[ok]), "last attempts")
        assert compared > 3000
    finally:
        a.close()
        b.close()


def _has_earlier_winner(made, kept):
    """per slot: a slot of the same node earlier in the list was kept"""
    seen, out = set(), np.zeros(len(made), dtype=bool)
    for i in range(len(made)):
        out[i] = made[i] >= 0 and int(made[i]) in seen
        if kept[i] >= 0:
            seen.add(int(kept[i]))
    return out


@pytest.mark.parametrize("form", ["device", "host"])
def test_the_chain_by_hand(rsa, O, form):
    """A sent in tick 0; B, deferred by A in tick 1, sent in tick 2 once A has left the air; C sent in tick 2; A again in tick 3 senses
    B's frame: deferred, its retry behind the batch: pending at tick 4"""
    c = SR.chain_run(O)
    eng = _engine(rsa, c.sc.nd, c.sc.params)
    try:
        out, n_exp = _csma(rsa, eng, c.sc, c.lists, 0, form, c.sc.threshold, c.p, air=c.AIR)
        _check(eng, c.run, out, n_exp, "chain, %s form" % form)
        a0, b1, c2, a3 = c.at
        assert (out["status"][a0], out["attempts"][a0], out["tick"][a0]) == (SR.SENT, 1, 0)
        assert (out["status"][b1], out["attempts"][b1], out["tick"][b1], out["flags"][b1]) == (SR.SENT, 2, 2, 0) and out["pkt"][b1] >= len(c.lists[2])
        assert (out["status"][c2], out["attempts"][c2], out["tick"][c2]) == (SR.SENT, 1, 2)
        assert (out["status"][a3], out["attempts"][a3], out["tick"][a3], out["pkt"][a3]) == (SR.PENDING, 1, 4, -1) and out["flags"][a3] & R.ED_BUSY
        _window_is(eng, O, c.sc, c.run, 3, "chain")
    finally:
        eng.close()


def test_small_path(rsa, O):
    """10 candidates per tick over 6 ticks on an empty window: at most 180 slots, fewer than kEdSmallWindow (256) frames in all: the
    index without a grid"""
    sc = BR.scene(O, "multi")
    near = np.argsort((sc.nd.x - sc.nd.x[0]) ** 2 + (sc.nd.y - sc.nd.y[0]) ** 2)[:60].astype(np.int32)    # (close together: they defer each other)
    lists = [near[10 * k:10 * k + 10] for k in range(6)]
    p = SR.Params(2, 0, 1, 3)
    r = SR.Run(O, sc, lists, p)
    assert (r.status == SR.SENT).any() and (r.attempts > 1).any() and r.n_exp.sum() < 256
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        eng.profile_enable(1)
        out, n_exp = _csma(rsa, eng, sc, lists, 0, "device", sc.threshold, p)
        _check(eng, r, out, n_exp, "small path")
        assert _kernels(eng) == {k.replace("<true", "<false") for k in GRID}, _kernels(eng)
    finally:
        eng.close()


def test_edge_lists(rsa, O):
    """A tick with no own candidates that receives retries, an all-padding tick, device-list entries outside 0 .. n_nodes-1 (packets with
    status NONE), an empty batch tail; the same under a NaN threshold (only RM_ED_TRANSMITTING defers); all-padding lists."""
    sc = BR.scene(O, "multi")
    base = [s[:60] for s in sc.ticks]
    bad = base[3].copy()
    bad[[2, 9]] = sc.nd.n, -7
    again = np.concatenate([base[0][base[0] >= 0][:12], base[4][:20]])          # nodes of tick 0 once more, two ticks later
    empty = np.zeros(0, dtype=np.int32)
    lists = [base[0], empty, np.full(10, -1, dtype=np.int32), bad, again, base[5], empty, empty]
    p = SR.Params(3, 0, 1, 21)
    for thr, what in ((sc.threshold, "edge lists"), (NAN, "NaN threshold")):
        r = SR.Run(O, sc, lists, p, threshold=thr)
        assert r.n_exp[1] > 0 and r.n_exp[2] > 10
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            out, n_exp = _csma(rsa, eng, sc, lists, 0, "device", thr, p)
            _check(eng, r, out, n_exp, what)
            _window_is(eng, O, sc, r, len(lists) - 1, what)
            real = np.concatenate([(s >= 0) & (s < sc.nd.n) for s in lists])
            assert not out["status"][~real].any() and not out["attempts"][~real].any() and np.isnan(out["energy_dbm"][~real]).all()
            assert (out["pkt"][~real] == -1).all() and out["status"][real].all()
            if thr != thr:
                assert set(out["flags"].tolist()) <= {0, R.ED_TRANSMITTING} and (out["flags"] == R.ED_TRANSMITTING).any()
            else:
                assert (out["attempts"] > 1).any() and (out["status"] == SR.FAILED).any()
        finally:
            eng.close()
    pads = [np.full(7, -1, dtype=np.int32), np.full(3, -1, dtype=np.int32)]
    r = SR.Run(O, sc, pads, p)
    for form in ("device", "host"):
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            out, n_exp = _csma(rsa, eng, sc, pads, 0, form, sc.threshold, p)
            _check(eng, r, out, n_exp, "all padding, %s form" % form)
            assert not out["status"].any()
        finally:
            eng.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_null_outputs(rsa, O, form):
    """every output pointer NULL in turn, all NULL together, and (device form) a NULL rm_csma_result: the others are as ever"""
    sc = BR.scene(O, "multi")
    lists = [s[:80] for s in sc.ticks[:5]]
    p = SR.Params(2, 0, 1, 4)
    r = SR.Run(O, sc, lists, p)
    names = [f for f, _ in rsa.Engine.CSMA_FIELDS]
    cases = [[f for f in names if f != g] for g in names] + [[]]
    for fields in cases + ([None] if form == "device" else []):
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            out, n_exp = _csma(rsa, eng, sc, lists, 0, form, sc.threshold, p, fields=fields or [], no_out=fields is None)
            assert sorted(out) == sorted(fields or [])
            _check(eng, r, out, n_exp, "outputs %s" % fields)
        finally:
            eng.close()


def test_self_contained_ticks(rsa, O):
    """frames shorter than a tick's gap to the next sample and an empty window: the batch after the gate is the self-contained form"""
    sc = BR.scene(O, "multi")
    lists = sc.ticks[:5]
    p = SR.Params(2, 0, 1, 4)
    r = SR.Run(O, sc, lists, p, air=500)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        out, n_exp = _csma(rsa, eng, sc, lists, 0, "device", sc.threshold, p, air=500)
        _check(eng, r, out, n_exp, "self-contained")
        real = np.concatenate(lists) >= 0
        assert (out["status"][real] == SR.SENT).all() and (out["attempts"][real] == 1).all() and eng.air_batch_stats()[0] == 0
    finally:
        eng.close()


def test_reception_stage_after_a_csma_batch(rsa, O):
    """rm_events_enable, a CSMA-CA batch, rm_events_process_batch: every tick's drain against O.Sim fed with the KEPT frames only, under
    packet numbers that count every slot of the expanded lists"""
    from test_gpu_events_batch import oracle_drain, same_drain
    sc, r = BR.scene(O, "multi"), SR.run(O, "multi")
    eng = _engine(rsa, sc.nd, sc.params)
    sim = O.Sim(sc.nd.n)
    try:
        eng.set_time(0)
        eng.events_enable()
        base = delivered = 0
        out, n_exp = _csma(rsa, eng, sc, r.lists, 0, "device", sc.threshold, SR.SCENES["multi"][1])
        _same_packets(out, r, "multi")
        ends = _times(sc, 0, len(r.lists))[1]
        views = eng.events_process_batch(ends)
        for k in range(len(r.lists)):
            exp = r.exp[k]
            raw = exp.raw
            for q, slot in enumerate(exp.slots):       # one packet at a time, in packet order, under its slot's number
                sel = slice(*np.searchsorted(raw.pkt, [q, q + 1]))
                one = O.TickResult(sel.stop - sel.start, np.zeros(sel.stop - sel.start, dtype=np.int32), raw.dst[sel], raw.verdict[sel],
                                   raw.rssi[sel], raw.sinr[sel], None, None, 0)
                sim.medium_calls(one, exp.new[q:q + 1], pkt_base=base + int(slot))
            base += int(r.n_exp[k])
            delivered += same_drain(views[k], oracle_drain(O, sim, ends[k]), "tick %d" % k)
        delivered += same_drain(eng.events_process(10 ** 6), oracle_drain(O, sim, 10 ** 6), "final drain")
        assert sim.pending == 0 and delivered > 500 and eng.events_next_packet() == base
        eng.events_disable()
    finally:
        sim.close()
        eng.close()


def test_refusals(rsa, O):
    """E8's refusals, each followed by a plain tick that gives what it gives on an untouched context: the parameters; what E7 refuses,
    with E7's codes; the 8192-candidate limit of an overlapping tick met by n_exp, not by n_src"""
    from radio_sim_amd import _lib
    from util import KINDS
    sc = BR.scene(O, "multi")
    nd = sc.nd
    eng = _engine(rsa, nd, sc.params)
    chain = CR.Chain(O, nd, sc.model(O))
    state = {"k": 0}
    good = SR.Params(2, 0, 1, 4)

    def after(what):
        k = state["k"]
        t0, _, ts = sc.times(k)
        src = sc.ticks[k % 12][:30]
        dev = DeviceArray(src)
        try:
            eng.tick_run_sources_device(t0, t0 + CR.TICK, dev.ptr.value, len(src), ts, CR.AIR)
            _same_links(eng.result_copy(len(src), cap=1 << 22), chain.plain_tick(t0, src, ts, CR.AIR), what + ": the plain tick that follows")
        finally:
            dev.free()
        state["k"] = k + 1

    def refused(code, form, what, p=good, reserved=None, lists=None, tc=None, air=None):
        k = state["k"]
        lists = [sc.ticks[(k + i) % 12] for i in range(3)] if lists is None else lists
        tb, te, c, ts = _times(sc, k, k + len(lists))
        c = tc(list(c)) if tc else c
        airs = air if air else [CR.AIR] * len(lists)
        par = _params(rsa, p, reserved)

        def call():
            if form == "host":
                return eng.batch_run_sources_csma(tb, te, lists, ts, airs, c, -90.0, par)
            d = [DeviceArray(np.ascontiguousarray(x, dtype=np.int32)) for x in lists]
            try:
                eng.batch_run_sources_csma_device(tb, te, [x.ptr.value for x in d], [len(x) for x in lists], ts, airs, c, -90.0, par)
            finally:
                for x in d:
                    x.free()
        _refused(rsa, eng, code, call)
        after("%s, %s form" % (what, form))

    def put(i, v):
        def f(lst):
            lst[i] = v(lst) if callable(v) else v
            return lst
        return f

    try:
        after("first tick")
        for form in ("host", "device"):
            for bad in (SR.Params(6, 1, 3, 0), SR.Params(-1, 1, 3, 0), SR.Params(2, 4, 3, 0), SR.Params(2, 0, 9, 0), SR.Params(2, -1, 3, 0)):
                refused(_lib.RM_ERR_INVALID, form, "parameters %s" % (bad.key(),), p=bad)
            refused(_lib.RM_ERR_INVALID, form, "reserved != 0", reserved=5)
            refused(_lib.RM_ERR_INVALID, form, "a sample before its tick's t_begin", tc=put(1, lambda c: c[1] - 129))
            refused(_lib.RM_ERR_INVALID, form, "a sample after its tick's start", tc=put(1, lambda c: c[1] + 73))
            refused(_lib.RM_ERR_INVALID, form, "an air time of 2^32 us", air=[CR.AIR, 2 ** 32, CR.AIR])
            refused(_lib.RM_ERR_INVALID, form, "a negative air time", air=[CR.AIR, -1, CR.AIR])
            # two ticks of 5000: n_src is within the limit, n_exp[1] = 10000 is not
            two = [np.arange(5000, dtype=np.int32), np.arange(5000, dtype=np.int32)[::-1].copy()]
            refused(_lib.RM_ERR_STATE, form, "an overlapping tick whose expanded list has more than 8192 slots", p=SR.Params(1, 0, 0, 1), lists=two)
        k = state["k"]                                          # (a good batch in between: the refusals left nothing behind)
        lists = [sc.ticks[(k + i) % 12] for i in range(2)]
        r = SR.Run(O, sc, lists, good, chain=chain, first_tick=k)
        out, n_exp = _csma(rsa, eng, sc, lists, k, "device", sc.threshold, good)
        _check(eng, r, out, n_exp, "the batch after the refusals")
        state["k"] = k + 2
        bad = [lists[0].copy(), lists[1]]
        bad[0][3] = nd.n
        refused(_lib.RM_ERR_INVALID, "host", "a host index out of range", lists=[bad[0], bad[1], bad[1]])
        k = state["k"]
        eng.tick_begin(sc.times(k)[0], sc.times(k)[0] + CR.TICK)
        tb, te, tc, ts = _times(sc, k, k + 2)
        _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: eng.batch_run_sources_csma(tb, te, lists, ts, [CR.AIR] * 2, tc, -90.0, _params(rsa, good)))
        eng.enqueue_tx(17, sc.times(k)[0], CR.AIR)                                      # (the host tick goes on: one frame joins the window)
        eng.tick_flush()
        chain.plain_tick(sc.times(k)[0], np.array([17], dtype=np.int32), sc.times(k)[0], CR.AIR)
        after("between rm_tick_begin and rm_tick_flush")
    finally:
        eng.close()
    other = rsa.Engine(0)                                       # not the SINR medium
    try:
        other.upload_table(nd)
        other.set_model(KINDS["udgm"])
        tb, te, tc, ts = _times(sc, 0, 2)
        _refused(rsa, other, _lib.RM_ERR_STATE, lambda: other.batch_run_sources_csma(tb, te, sc.ticks[:2], ts, [CR.AIR] * 2, tc, -90.0, _params(rsa, good)))
    finally:
        other.close()


def test_e7_calls_still_give_e7_after_a_csma_batch(rsa, O):
    """the two gates share the context's buffers: a CSMA-CA batch, then the gated batch and the gated lone tick, against the chain"""
    sc = BR.scene(O, "multi")
    p = SR.SCENES["multi"][1]
    chain = CR.Chain(O, sc.nd, sc.model(O))
    r = SR.Run(O, sc, sc.ticks[:4], p, chain=chain)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        out, n_exp = _csma(rsa, eng, sc, r.lists, 0, "device", sc.threshold, p)
        _check(eng, r, out, n_exp, "CSMA batch")
        want = [chain.gated_tick(sc.times(k)[0], sc.ticks[k], sc.times(k)[2], CR.AIR, sc.times(k)[1], sc.threshold) for k in range(4, 8)]
        got = _batch(eng, sc, sc.ticks[4:7], 4, "device", sc.threshold)
        for b in range(3):
            _same_sense(got[b], want[b][:2], "E7 batch, tick %d" % (4 + b))
            _same_links(eng.batch_result_copy(b, len(sc.ticks[4 + b]), cap=1 << 22), want[b][2], "E7 batch, tick %d" % (4 + b))
        t0, tc, ts = sc.times(7)
        f, e = eng.tick_run_sources_cca(t0, t0 + CR.TICK, sc.ticks[7], ts, CR.AIR, tc, sc.threshold)
        _same_sense((f, e), want[3][:2], "E6 tick 7")
        _same_links(eng.result_copy(len(sc.ticks[7]), cap=1 << 22), want[3][2], "E6 tick 7")
        r2 = SR.Run(O, sc, sc.ticks[8:12], p, chain=chain, first_tick=8)
        out, n_exp = _csma(rsa, eng, sc, r2.lists, 8, "host", sc.threshold, p)
        _check(eng, r2, out, n_exp, "CSMA batch over a window of earlier calls")
    finally:
        eng.close()
