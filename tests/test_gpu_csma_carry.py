"""The carry of the CSMA-CA gated batch (rm_batch_run_sources_csma_carry*, rm_csma_carry_collect*) on the GPU.
The truth for every split is the oracle's run over the WHOLE tick range (tests/csma_ref.py::Run); tests/csma_carry_ref.py says what
each part reports, what it carries on and how the parts merge; tests/test_csma_carry_ref.py holds the scenes' conditions.  Everything
is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cca_batch_ref as BR
import cca_ref as CR
import csma_carry_ref as KR
import csma_ref as SR
import energy_ref as R
from test_gpu_cca import _bits, _engine, _same_links
from test_gpu_cca_batch import _refused, _times
from test_gpu_csma import SENTINEL, _csma, _params, _window_is
from util import DeviceArray

pytestmark = pytest.mark.gpu

FIELDS = ("status", "attempts", "tick", "pkt", "flags", "energy_dbm")
COLLECT = {"k_csma_collect<false>", "k_csma_collect_scan", "k_csma_collect<true>"}


def _part(rsa, eng, sc, lists, first, form, thr, p, carry, air=CR.AIR, fields=None, carried_fields=None, no_out=False, collect=True, cap=None):
    """ticks first .. of the scene's clock as ONE carry batch -> (own table, carried table, n_exp, carry-out or None), the carry-out
    collected in the matching form"""
    lists = [np.ascontiguousarray(s, dtype=np.int32) for s in lists]
    tb, te, tc, ts = _times(sc, first, first + len(lists))
    airs = [air] * len(lists)
    own_f = list(FIELDS) if fields is None else list(fields)
    car_f = list(FIELDS) if carried_fields is None else list(carried_fields)
    par = _params(rsa, p)
    n_carry = 0 if carry is None else len(carry)
    if form == "host":
        out, carried, n_exp = eng.batch_run_sources_csma_carry(tb, te, lists, ts, airs, tc, thr, par, carry, fields=own_f, carried_fields=car_f)
        nxt = rsa.Engine.csma_carry_collect(lists, tc, carry, out, carried, cap=cap) if collect else None
        return out, carried, n_exp, nxt
    total = sum(len(s) for s in lists)
    types = dict(rsa.Engine.CSMA_FIELDS)
    d_s = [DeviceArray(s) if len(s) else None for s in lists]
    d_o = {f: DeviceArray(np.full(max(total, 1), SENTINEL[f], dtype=types[f])) for f in own_f}
    d_c = {f: DeviceArray(np.full(max(n_carry, 1), SENTINEL[f], dtype=types[f])) for f in car_f}
    try:
        ptrs = [d.ptr.value if d else None for d in d_s]
        own_p, car_p = {f: d.ptr.value for f, d in d_o.items()}, {f: d.ptr.value for f, d in d_c.items()}
        n_exp = eng.batch_run_sources_csma_carry_device(tb, te, ptrs, [len(s) for s in lists], ts, airs, tc, thr, par, carry,
                                                        None if no_out else own_p, None if no_out else car_p)
        nxt = eng.csma_carry_collect_device(ptrs, [len(s) for s in lists], tc, carry, own_p, car_p, cap=cap) if collect else None
        eng.sync()
        for d, s in zip(d_s, lists):
            if d:
                np.testing.assert_array_equal(DeviceArray.read(d.ptr.value, np.int32, len(s)), s, err_msg="a caller's dev_src was written")
        out = {f: DeviceArray.read(d.ptr.value, types[f], max(total, 1))[:total] for f, d in d_o.items()}
        carried = {f: DeviceArray.read(d.ptr.value, types[f], max(n_carry, 1))[:n_carry] for f, d in d_c.items()}
        return out, carried, n_exp, nxt
    finally:
        for d in d_s + list(d_o.values()) + list(d_c.values()):
            if d:
                d.free()


def _same_table(got, want, what):
    for f, a in got.items():
        if f == "energy_dbm":
            np.testing.assert_array_equal(_bits(a), _bits(want[f]), err_msg="%s: energy bits" % what)
        else:
            np.testing.assert_array_equal(a, want[f], err_msg="%s: %s" % (what, f))


def _split_run(rsa, eng, O, sc, r, p, cuts, form, air=CR.AIR, links=True):
    """the whole run `r` issued on `eng` as consecutive carry batches cut at `cuts`, every part against what the oracle's whole run
    says of it: n_exp, every tick's links, both tables, the carry-out -> (the merged outcome, the parts' tables)"""
    n_ticks = len(r.lists)
    t_cca = [sc.times(k)[1] for k in range(n_ticks)]
    edges = [0] + list(cuts) + [n_ticks]
    m = KR.Merge(len(r.status))
    carry, seen = None, []
    for first, last in zip(edges[:-1], edges[1:]):
        what = "%s form, ticks %d .. %d" % (form, first, last - 1)
        want_carry, ids = KR.carry_at(r, first, t_cca)
        carry = want_carry[:0] if carry is None else carry
        np.testing.assert_array_equal(carry, want_carry, err_msg=what + ": the carry-in is not what the whole run carries over the cut")
        lists = r.lists[first:last]
        out, carried, n_exp, nxt = _part(rsa, eng, sc, lists, first, form, sc.threshold, p, carry, air=air)
        alive = KR.live(r, first, last, ids)                    # (the whole's slots without the dead ones of packets from before the cut)
        np.testing.assert_array_equal(n_exp, [len(a) for a in alive], err_msg=what + ": n_exp")
        if links:
            for b in range(last - first):
                _same_links(eng.batch_result_copy(b, int(n_exp[b]), cap=1 << 22), KR.expected_links(r.exp[first + b], alive[b]),
                            "%s, tick %d" % (what, first + b))
        own_w, car_w = KR.tables_of(r, first, last, ids, want_carry)
        _same_table(out, own_w, what + ", own table")
        _same_table(carried, car_w, what + ", carried table")
        want_nxt, who = KR.collect(lists, t_cca[first:last], carry, out, carried)
        np.testing.assert_array_equal(nxt, want_nxt, err_msg=what + ": carry-out")
        m.part(first, sum(len(s) for s in lists), out, carried, who)
        seen.append((out, carried, n_exp))
        carry = nxt
    want = r.outcome()
    want[3] = KR.whole_pkt(r, cuts)
    np.testing.assert_array_equal(m.outcome(), want, err_msg="the merged parts are not the whole")
    np.testing.assert_array_equal(_bits(m.energy), _bits(r.energy), err_msg="the merged parts are not the whole: energy bits")
    return m, seen


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("name,cuts", [("multi", (6,)), ("multi", (4, 8)), ("ch16", (5,))])
def test_splits_equal_the_whole(rsa, O, name, cuts, form):
    """multi 6 + 6 and 4 + 4 + 4 (289 packets carried twice, 17 carried in with their next attempt behind part 2), ch16 5 + 6 (2452
    carried: k_csma_collect over ten workgroups, carried slots at positions above 1024 of the resolve pass)"""
    sc, r = BR.scene(O, name), SR.run(O, name)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        eng.profile_enable(1)
        m, _ = _split_run(rsa, eng, O, sc, r, SR.SCENES[name][1], cuts, form)
        _window_is(eng, O, sc, r, len(r.lists) - 1, "%s %s, %s form" % (name, cuts, form))
        names = {k for k in eng.profile_kernels() if k.startswith("k_csma_collect")}
        assert names == (COLLECT if form == "device" else set()), names
        if len(cuts) == 2:
            assert (m.times_carried >= 2).sum() >= 5
    finally:
        eng.close()


def test_same_whole_from_the_engine(rsa, O):
    """the unsplit rm_batch_run_sources_csma on a second context against the split on the first: outcomes and links"""
    sc, r = BR.scene(O, "multi"), SR.run(O, "multi")
    p = SR.SCENES["multi"][1]
    a, b = _engine(rsa, sc.nd, sc.params), _engine(rsa, sc.nd, sc.params)
    try:
        whole, n_exp = _csma(rsa, b, sc, r.lists, 0, "device", sc.threshold, p)
        t_cca = [sc.times(k)[1] for k in range(12)]
        m, carry = KR.Merge(len(r.status)), None
        for first, last in ((0, 6), (6, 12)):
            out, carried, n_part, nxt = _part(rsa, a, sc, r.lists[first:last], first, "device", sc.threshold, p, carry)
            alive = KR.live(r, first, last, KR.carry_at(r, first, t_cca)[1])
            np.testing.assert_array_equal(n_part, [len(x) for x in alive])
            for k in range(first, last):
                ra, rb = a.batch_result_copy(k - first, int(n_part[k - first]), cap=1 << 22), b.batch_result_copy(k, int(n_exp[k]), cap=1 << 22)
                assert ra.count == rb.count > 0
                live_k = alive[k - first]                       # the whole's packet numbers of the part's slots
                np.testing.assert_array_equal(live_k[ra.pkt], rb.pkt, err_msg="tick %d: pkt" % k)
                np.testing.assert_array_equal(np.diff(ra.pkt_offset.astype(np.int64)), np.diff(rb.pkt_offset.astype(np.int64))[live_k],
                                              err_msg="tick %d: pkt_offset" % k)
                np.testing.assert_array_equal(ra.pkt_interference, rb.pkt_interference[live_k], err_msg="tick %d: Tx-failure flags" % k)
                for f in ("dst", "verdict"):
                    np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg="tick %d: %s" % (k, f))
                for f in ("rssi", "sinr"):
                    np.testing.assert_array_equal(_bits(getattr(ra, f)), _bits(getattr(rb, f)), err_msg="tick %d: %s" % (k, f))
            m.part(first, 900, out, carried, KR.collect(r.lists[first:last], t_cca[first:last], carry if carry is not None else [], out, carried)[1])
            carry = nxt
        got = {"status": m.status, "attempts": m.attempts, "tick": m.tick, "pkt": m.pkt, "flags": m.flags, "energy_dbm": m.energy}
        sent = whole["status"] == SR.SENT
        np.testing.assert_array_equal(whole["pkt"][sent], r.pkt[sent])
        whole["pkt"] = KR.whole_pkt(r, (6,))
        _same_table(got, whole, "split against the engine's whole")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_no_carry_is_the_csma_batch(rsa, O, form):
    sc = BR.scene(O, "multi")
    lists, p = sc.ticks[:5], SR.SCENES["multi"][1]
    a, b = _engine(rsa, sc.nd, sc.params), _engine(rsa, sc.nd, sc.params)
    try:
        out, carried, n_exp, nxt = _part(rsa, a, sc, lists, 0, form, sc.threshold, p, None)
        want, n_want = _csma(rsa, b, sc, lists, 0, form, sc.threshold, p)
        np.testing.assert_array_equal(n_exp, n_want)
        _same_table(out, want, "n_carry = 0")
        assert all(len(v) == 0 for v in carried.values()) and (out["status"] == SR.PENDING).sum() == len(nxt) > 5
        for k in range(len(lists)):
            ra, rb = a.batch_result_copy(k, int(n_exp[k]), cap=1 << 22), b.batch_result_copy(k, int(n_exp[k]), cap=1 << 22)
            assert ra.count == rb.count > 0
            for f in ("pkt", "dst", "verdict", "pkt_interference", "pkt_offset"):
                np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg="tick %d: %s" % (k, f))
            for f in ("rssi", "sinr"):
                np.testing.assert_array_equal(_bits(getattr(ra, f)), _bits(getattr(rb, f)), err_msg="tick %d: %s" % (k, f))
    finally:
        a.close()
        b.close()


NEAR_AIR = 2900


def _near_run(O):
    """60 nodes close together, 10 per tick over 3 ticks, then 3 ticks without own candidates; frames of 2900 us (on the air at the next
    two ticks' samples, gone at the third), every retry within two ticks, two backoffs: cut after tick 3 the second part has empty own
    lists and only carried packets -- by the oracle 20 of them, of which 15 end sent and 5 fail inside it"""
    if "carry-near" not in SR._CACHE:
        sc = BR.scene(O, "multi")
        near = np.argsort((sc.nd.x - sc.nd.x[0]) ** 2 + (sc.nd.y - sc.nd.y[0]) ** 2)[:60].astype(np.int32)
        empty = np.zeros(0, dtype=np.int32)
        lists = [near[0:10], near[10:20], near[20:30], empty, empty, empty]
        p = SR.Params(2, 0, 1, 3)
        SR._CACHE["carry-near"] = (sc, lists, p, SR.Run(O, sc, lists, p, air=NEAR_AIR))
    return SR._CACHE["carry-near"]


@pytest.mark.parametrize("form", ["device", "host"])
def test_only_carried_packets(rsa, O, form):
    """a batch with empty own lists and only carried packets; max_backoffs reached inside the carried part: FAILED with max_backoffs + 1
    attempts in all"""
    sc, lists, p, r = _near_run(O)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        ids = KR.carry_at(r, 3, [sc.times(k)[1] for k in range(len(lists))])[1]
        fate = r.status[np.array(ids, dtype=np.int64)]          # (the scene's conditions, from the oracle alone)
        assert len(ids) >= 5 and (fate == SR.SENT).sum() >= 2 and (fate == SR.FAILED).sum() >= 2
        m, seen = _split_run(rsa, eng, O, sc, r, p, (3,), form, air=NEAR_AIR)
        carried = seen[1][1]
        failed = carried["status"] == SR.FAILED
        assert len(carried["status"]) >= 3 and failed.any() and (carried["attempts"][failed] == p.max_backoffs + 1).all()
        assert (carried["status"] == SR.SENT).any()
        _window_is(eng, O, sc, r, len(lists) - 1, "only carried packets")
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_the_chain_split_after_tick_1(rsa, O, form):
    """the hand-built chain: B, deferred by A in tick 1, is carried and sent in what is now tick 0 of the second part"""
    c = SR.chain_run(O)
    eng = _engine(rsa, c.sc.nd, c.sc.params)
    try:
        m, seen = _split_run(rsa, eng, O, c.sc, c.run, c.p, (2,), form, air=c.AIR)
        a0, b1, c2, a3 = c.at
        t_cca = [c.sc.times(k)[1] for k in range(4)]
        _, ids = KR.carry_at(c.run, 2, t_cca)
        at = ids.index(b1)
        carried = seen[1][1]
        assert (carried["status"][at], carried["attempts"][at], carried["tick"][at], carried["flags"][at]) == (SR.SENT, 2, 0, 0)
        assert carried["pkt"][at] >= len(c.lists[2])
        assert (m.status[a3], m.tick[a3]) == (SR.PENDING, 4)
        _window_is(eng, O, c.sc, c.run, 3, "chain")
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_smallest_shapes(rsa, O, form):
    """one tick over an empty window, carried packets written by hand: one carried packet; two of one node (the first wins, the second
    gets RM_ED_TRANSMITTING); a carried packet and an own entry of one node (the own entry wins); carried packets behind the batch only,
    with and without own candidates"""
    sc = BR.scene(O, "multi")
    p = SR.Params(2, 1, 3, 5)
    t0, tc, ts = sc.times(0)
    j, other = int(sc.ticks[0][0]), int(sc.ticks[0][1])
    origin = -3000 + sc.times(0)[1]                             # (a tick three before the scene's clock began)
    chain = CR.Chain(O, sc.nd, sc.model(O))
    clear = chain.sense(np.array([j], dtype=np.int32), tc, sc.threshold)
    assert clear[0][0] == 0

    def nxt(slot, a):                                           # the tick of attempt a + 1 after attempt a in tick 0
        return 1 + SR.backoff(p, origin, slot, a)

    def run(own, rows, kept):
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            out, carried, n_exp, _ = _part(rsa, eng, sc, [np.array(own, dtype=np.int32)], 0, form, sc.threshold, p, KR.carry_list(rows))
            want = CR.Chain(O, sc.nd, sc.model(O)).plain_tick(t0, np.array(kept, dtype=np.int32), ts, CR.AIR)
            assert n_exp[0] == len(kept)
            if len(kept):
                _same_links(eng.batch_result_copy(0, len(kept), cap=1 << 22), want, "smallest shapes")
            return out, carried
        finally:
            eng.close()

    def entry(t, i):
        return tuple(int(t[f][i]) for f in ("status", "attempts", "tick", "pkt", "flags"))

    out, car = run([], [(origin, 4, j, 0, 1)], [j])
    assert entry(car, 0) == (SR.SENT, 2, 0, 0, 0) and _bits(car["energy_dbm"])[0] == _bits(clear[1])[0]
    out, car = run([], [(origin, 4, j, 0, 1), (origin, 9, j, 0, 2)], [j, -1])
    assert entry(car, 0) == (SR.SENT, 2, 0, 0, 0)
    assert entry(car, 1) == (SR.FAILED, 3, -1, -1, R.ED_TRANSMITTING) and _bits(car["energy_dbm"])[1] == _bits(clear[1])[0]
    out, car = run([other], [(origin, 4, j, 0, 1), (origin, 9, j, 0, 1)], [other, j, -1])
    assert entry(car, 1) == (SR.PENDING, 2, nxt(9, 1), -1, R.ED_TRANSMITTING)
    out, car = run([j], [(origin, 4, j, 0, 1)], [j, -1])
    assert entry(out, 0) == (SR.SENT, 1, 0, 0, 0) and entry(car, 0) == (SR.PENDING, 2, nxt(4, 1), -1, R.ED_TRANSMITTING)
    for own in ([], [j, other]):
        out, car = run(own, [(origin, 4, j, 1, 1), (origin, 9, other, 700, 2)], own)
        assert entry(car, 0) == (SR.PENDING, 1, 1, -1, 0) and entry(car, 1) == (SR.PENDING, 2, 700, -1, 0) and np.isnan(car["energy_dbm"]).all()
        assert all(entry(out, i) == (SR.SENT, 1, 0, i, 0) for i in range(len(own)))


@pytest.mark.parametrize("form", ["device", "host"])
def test_null_outputs(rsa, O, form):
    """every output pointer of both tables NULL in turn, all NULL together, and (device form) both rm_csma_result NULL: the others and
    the links are as ever"""
    sc = BR.scene(O, "multi")
    lists = [s[:80] for s in sc.ticks[:5]]
    p = SR.Params(2, 0, 1, 4)
    key = "carry-null"
    if key not in SR._CACHE:
        SR._CACHE[key] = SR.Run(O, sc, lists, p)
    r = SR._CACHE[key]
    t_cca = [sc.times(k)[1] for k in range(5)]
    carry, ids = KR.carry_at(r, 2, t_cca)
    own_w, car_w = KR.tables_of(r, 2, 5, ids, carry)
    assert len(carry) >= 5
    cases = [[f for f in FIELDS if f != g] for g in FIELDS] + [[]]
    for fields in cases + ([None] if form == "device" else []):
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            _part(rsa, eng, sc, lists[:2], 0, form, sc.threshold, p, None, collect=False)
            out, carried, n_exp, _ = _part(rsa, eng, sc, lists[2:], 2, form, sc.threshold, p, carry, fields=fields or [], carried_fields=fields or [],
                                           no_out=fields is None, collect=False)
            assert sorted(out) == sorted(carried) == sorted(fields or [])
            alive = KR.live(r, 2, 5, ids)
            np.testing.assert_array_equal(n_exp, [len(a) for a in alive])
            _same_table(out, own_w, "outputs %s, own" % fields)
            _same_table(carried, car_w, "outputs %s, carried" % fields)
            for b in range(3):
                _same_links(eng.batch_result_copy(b, int(n_exp[b]), cap=1 << 22), KR.expected_links(r.exp[2 + b], alive[b]),
                            "outputs %s, tick %d" % (fields, 2 + b))
        finally:
            eng.close()


def test_refusals(rsa, O):
    """E9's own refusals in both forms, each followed by a plain tick that gives what it gives on an untouched context, and at the end an
    E8 batch against the oracle's chain"""
    from radio_sim_amd import _lib
    sc = BR.scene(O, "multi")
    nd = sc.nd
    eng = _engine(rsa, nd, sc.params)
    chain = CR.Chain(O, nd, sc.model(O))
    state = {"k": 0}
    p = SR.Params(2, 0, 1, 4)
    good = (128, 3, 7, 0, 1)

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

    def refused(code, form, what, carry=None, lists=None, raw_n=None, par=p):
        k = state["k"]
        lists = [sc.ticks[(k + i) % 12] for i in range(3)] if lists is None else lists
        tb, te, tc, ts = _times(sc, k, k + len(lists))
        airs = [CR.AIR] * len(lists)

        def call():
            if raw_n is not None:                               # n_carry itself: past the wrapper
                a = [np.ascontiguousarray(x, dtype=np.int64) for x in (tb, te, ts, airs, tc)]
                cnt = np.array([len(x) for x in lists], dtype=np.int32)
                if form == "host":
                    ptrs, fn = np.array([x.ctypes.data for x in lists], dtype=np.uint64), eng._L.rm_batch_run_sources_csma_carry
                    _lib.check(fn(eng._h, len(lists), a[0].ctypes.data, a[1].ctypes.data, ptrs.ctypes.data, cnt.ctypes.data, a[2].ctypes.data,
                                  a[3].ctypes.data, a[4].ctypes.data, -90.0, C.byref(_params(rsa, par)), None, None, None, raw_n, None))
                    return
                d = [DeviceArray(np.ascontiguousarray(x, dtype=np.int32)) for x in lists]
                try:
                    ptrs, fn = np.array([x.ptr.value for x in d], dtype=np.uint64), eng._L.rm_batch_run_sources_csma_carry_device
                    _lib.check(fn(eng._h, len(lists), a[0].ctypes.data, a[1].ctypes.data, ptrs.ctypes.data, cnt.ctypes.data, a[2].ctypes.data,
                                  a[3].ctypes.data, a[4].ctypes.data, -90.0, C.byref(_params(rsa, par)), None, None, None, raw_n, None))
                finally:
                    for x in d:
                        x.free()
                return
            if form == "host":
                return eng.batch_run_sources_csma_carry(tb, te, lists, ts, airs, tc, -90.0, _params(rsa, par), carry)
            d = [DeviceArray(np.ascontiguousarray(x, dtype=np.int32)) for x in lists]
            try:
                eng.batch_run_sources_csma_carry_device(tb, te, [x.ptr.value for x in d], [len(x) for x in lists], ts, airs, tc, -90.0,
                                                        _params(rsa, par), carry)
            finally:
                for x in d:
                    x.free()
        _refused(rsa, eng, code, call)
        after("%s, %s form" % (what, form))

    def row(field, v):
        bad = list(good)
        bad[field] = v
        return KR.carry_list([good, tuple(bad)])

    try:
        after("first tick")
        for form in ("host", "device"):
            refused(_lib.RM_ERR_INVALID, form, "n_carry < 0", raw_n=-1)
            refused(_lib.RM_ERR_INVALID, form, "n_carry > 0 without a list", raw_n=2)
            refused(_lib.RM_ERR_INVALID, form, "a node of n_nodes", carry=row(2, nd.n))
            refused(_lib.RM_ERR_INVALID, form, "a node of -1", carry=row(2, -1))
            refused(_lib.RM_ERR_INVALID, form, "attempt 0", carry=row(4, 0))
            refused(_lib.RM_ERR_INVALID, form, "attempt max_backoffs + 1", carry=row(4, 3))
            refused(_lib.RM_ERR_INVALID, form, "a negative tick", carry=row(3, -1))
            refused(_lib.RM_ERR_INVALID, form, "a negative origin_slot", carry=row(1, -1))
            refused(_lib.RM_ERR_INVALID, form, "E8's own: parameters out of range", carry=KR.carry_list([good]), par=SR.Params(6, 1, 3, 0))
            # 5000 own candidates and 5000 carried attempts in one overlapping tick: n_src is within the 8192 limit, n_exp[0] is not
            many = KR.carry_list([(128, k, k, 0, 1) for k in range(5000)])
            refused(_lib.RM_ERR_STATE, form, "an overlapping tick of more than 8192 slots, carried ones included", carry=many,
                    lists=[np.arange(5000, dtype=np.int32), np.arange(10, dtype=np.int32)])
        # packets and carried packets together above 2^27: the lengths alone decide (nothing of the list is read before the refusal)
        k = state["k"]
        tb, te, tc, ts = _times(sc, k, k + 1)
        dev = DeviceArray(np.zeros(16, dtype=np.int32))
        try:
            _refused(rsa, eng, _lib.RM_ERR_CAPACITY, lambda: eng.batch_run_sources_csma_carry_device(
                tb, te, [dev.ptr.value], [1 << 27], ts, [CR.AIR], tc, -90.0, _params(rsa, p), KR.carry_list([good])))
        finally:
            dev.free()
        after("2^27 packets and one carried")
        k = state["k"]                                          # an E8 batch: the refusals left nothing behind
        lists = [sc.ticks[(k + i) % 12] for i in range(2)]
        r = SR.Run(O, sc, lists, p, chain=chain, first_tick=k)
        out, n_exp = _csma(rsa, eng, sc, lists, k, "device", sc.threshold, p)
        np.testing.assert_array_equal(n_exp, r.n_exp)
        _same_table(out, {"status": r.status, "attempts": r.attempts, "tick": r.tick, "pkt": r.pkt, "flags": r.flags, "energy_dbm": r.energy},
                    "the E8 batch after the refusals")
        for b in range(2):
            _same_links(eng.batch_result_copy(b, int(n_exp[b]), cap=1 << 22), r.exp[b], "the E8 batch after the refusals, tick %d" % b)
    finally:
        eng.close()


def test_collect_cap(rsa, O):
    """rm_csma_carry_collect_device with too small a cap: RM_ERR_CAPACITY and the count; with just enough: the carry-out"""
    from radio_sim_amd import _lib
    sc, r = BR.scene(O, "multi"), SR.run(O, "multi")
    p = SR.SCENES["multi"][1]
    t_cca = [sc.times(k)[1] for k in range(12)]
    want, _ = KR.carry_at(r, 6, t_cca)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        for cap, ok in ((len(want) - 1, False), (0, False), (len(want), True)):
            if ok:
                np.testing.assert_array_equal(_part(rsa, eng, sc, r.lists[:6], 0, "device", sc.threshold, p, None, cap=cap)[3], want)
                continue
            with pytest.raises(rsa.RadioMediumError) as err:
                _part(rsa, eng, sc, r.lists[:6], 0, "device", sc.threshold, p, None, cap=cap)
            assert err.value.code == _lib.RM_ERR_CAPACITY and err.value.count == len(want)
            eng.close()
            eng = _engine(rsa, sc.nd, sc.params)
    finally:
        eng.close()
