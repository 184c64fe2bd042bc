"""The unicast outcome query (rm_unicast_query*, rm_unicast.hip) on the GPU.  Expected values come from
tests/unicast_ref.py alone (the spec's table over the oracle's per-tick results; tests/test_unicast_ref.py holds the scenes'
conditions for that reference).  Every comparison is exact: status, link, rssi bits, sinr bits, reply_src."""
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
import stats_ref as S
import unicast_ref as U
from test_gpu_cca_batch import _batch as _gated_batch
from test_gpu_csma import _csma
from test_gpu_csma_carry import _part
from test_gpu_stats import _engine, _lone, _run_batch
from util import DeviceArray, configure_engine, to_tx_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK = R.TICK
INVALID, CAPACITY, STATE = -1, -4, -5
TYPES = {"status": np.uint8, "link": np.int32, "rssi": np.float64, "sinr": np.float64, "reply_src": np.int32}
SENTINEL = {"status": 0xEE, "link": -777, "rssi": 12345.0, "sinr": 54321.0, "reply_src": -778}

_REF = {}


def _ref(key, make):
    """a scene's reference slots: computed once, shared and left unchanged"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _lone_ref(em_seed=None):
    nd, srcs, start, air = R.scene_lone()
    return nd, srcs, start, air, _ref(("lone", em_seed), lambda: U.sinr_slots(nd, [srcs], [start], air, em_seed))


def _batch_ref(overlap, em_seed=None):
    nd, lists, starts, air = R.scene_batch(overlap)
    return nd, lists, starts, air, _ref(("batch", overlap, em_seed), lambda: U.sinr_slots(nd, lists, starts, air, em_seed))


class _DevOut:
    """the five outputs in device memory, one entry more than asked for: the query must leave it alone"""

    def __init__(self, n, fields=U.FIELDS):
        self.n = n
        self.d = {f: DeviceArray(np.full(n + 1, SENTINEL[f], dtype=TYPES[f])) for f in fields}

    def ptrs(self):
        return {f: d.ptr.value for f, d in self.d.items()}

    def read(self, written=True):
        out = {}
        for f, d in self.d.items():
            a = DeviceArray.read(d.ptr.value, TYPES[f], self.n + 1)
            guard = np.full(1, SENTINEL[f], dtype=TYPES[f])
            assert a[-1:].tobytes() == guard.tobytes(), "the query wrote behind its %s array" % f
            if not written:
                assert a.tobytes() == np.full(self.n + 1, SENTINEL[f], dtype=TYPES[f]).tobytes(), "a refused query wrote to " + f
            out[f] = a[:-1]
        return out

    def free(self):
        for d in self.d.values():
            d.free()


def _query(eng, form, want_lists, fields=U.FIELDS):
    """the slots form -> dict of flat arrays (device: through device arrays, the wanted list checked to be unwritten)"""
    if form == "host":
        return eng.unicast_query(want_lists, fields=fields)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(w, dtype=np.int32) for w in want_lists]), dtype=np.int32)
    d_w, out = DeviceArray(flat), _DevOut(len(flat), fields)
    try:
        eng.unicast_query_device([len(w) for w in want_lists], d_w.ptr.value, out.ptrs())
        eng.sync()
        np.testing.assert_array_equal(DeviceArray.read(d_w.ptr.value, np.int32, max(len(flat), 1))[:len(flat)], flat)
        return out.read()
    finally:
        d_w.free()
        out.free()


def _query_at(eng, form, slot, pkt, want):
    slot, pkt, want = (np.ascontiguousarray(a, dtype=np.int32) for a in (slot, pkt, want))
    if form == "host":
        return eng.unicast_query_at(slot, pkt, want)
    d, out = [DeviceArray(a) for a in (slot, pkt, want)], _DevOut(len(want))
    try:
        eng.unicast_query_at_device(len(want), d[0].ptr.value, d[1].ptr.value, d[2].ptr.value, out.ptrs())
        eng.sync()
        return out.read()
    finally:
        for x in d:
            x.free()
        out.free()


def _expected(slots, want_lists, lost=()):
    return U.flat([s.outcome(w, lost=(b in lost)) for b, (s, w) in enumerate(zip(slots, want_lists))])


def _both_forms(eng, slots, what, lost=()):
    """the pick rule over the slots through the device form (out-of-range nodes included) and the host form"""
    for form in ("host", "device"):
        want = U.wants(slots, host=(form == "host"))
        exp = _expected(slots, want, lost)
        U.equal(_query(eng, form, want), exp, "%s, %s form" % (what, form))
    return exp   # (the device form's: the pick rule as it is)


# ---- 4. the lone forms on the SINR medium -----------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["flush", "view", "sources"])
def test_lone_forms(rsa, O, form):
    nd, srcs, start, air, slots = _lone_ref(R.SEED)
    eng, d = _engine(rsa, nd, stats=False, em_seed=R.SEED), DeviceArray(srcs)
    try:
        got = _lone(eng, form, d, srcs, start, air)
        np.testing.assert_array_equal(got.dst, slots[0].dst)          # the links are the oracle's
        np.testing.assert_array_equal(got.verdict, slots[0].verdict)
        exp = _both_forms(eng, slots, "lone tick by " + form)
        c = U.counts(exp["status"])
        assert min(c[U.UNHEARD], c[U.INTERFERED], c[U.DELIVERED]) >= 8
        # the at-form over a lone tick: slot 0, any other slot is NONE
        want = U.wants(slots)[0]
        n = len(want)
        slot = np.where(np.arange(n) % 7 == 6, np.array([1, -1, 512, 2 ** 30])[np.arange(n) % 4], 0).astype(np.int32)
        pkt = np.arange(n, dtype=np.int32)
        exp_at = slots[0].outcome(np.where(slot == 0, want, -1))
        for qform in ("device", "host"):
            w = np.where(want >= nd.n, -1, want) if qform == "host" else want
            U.equal(_query_at(eng, qform, slot, pkt, w), slots[0].outcome(np.where(slot == 0, w, -1)), "at-form, " + qform)
        assert (exp_at["status"][slot != 0] == U.NONE).all()
    finally:
        d.free()
        eng.close()


# ---- 5. the four reference media ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["udgm", "udgm_const", "n2n"])
def test_reference_media(rsa, O, name):
    scene = getattr(S, "scene_" + name)()
    nd, kind, params, pk, matrix, seed = scene
    s = _ref(("media", name), lambda: U.media_slot(scene))
    eng = rsa.Engine(0)
    try:
        configure_engine(eng, nd, kind, params, matrix)
        if seed is not None:
            eng.seed(seed)
        gpu = eng.tick(to_tx_records(rsa, pk), cap=1 << 20)
        np.testing.assert_array_equal(gpu.dst, s.dst)
        np.testing.assert_array_equal(gpu.verdict, s.verdict)
        if seed is not None:
            assert s.res.pkt_draws.sum() > 0 and eng.rng_state == s.res.rng_state     # the verdicts came from draws
        exp = _both_forms(eng, [s], name)
        assert np.isnan(exp["sinr"]).all()                                            # no SINR column on these media
        if seed is not None:
            assert eng.rng_state == s.res.rng_state                                   # the query left the generator alone
    finally:
        eng.close()


def test_null_medium_through_the_dense_tick(rsa, O):
    scene = S.scene_null()
    nd, kind, params, pk, _, _ = scene
    s = _ref(("media", "null"), lambda: U.media_slot(scene))
    srcs = np.ascontiguousarray(pk["src"], dtype=np.int32)
    # first and last node, the nodes at the lane (64) and cell (1024) boundaries, per frame; then the pick rule
    edge = np.array([0, nd.n - 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, nd.n - 2, 1], dtype=np.int32)
    eng, d = rsa.Engine(0), DeviceArray(srcs)
    try:
        configure_engine(eng, nd, kind, params)
        eng.set_link_capacity(1 << 20)
        for k in range(0, len(edge), 2):
            eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, S.AIR)   # (a fresh dense tick: its records are laid out on request)
            if os.environ.get("RM_DENSE_TICK") != "0":
                assert eng.result_dense().n_packets == len(srcs)
            want = np.where(np.arange(len(srcs)) % 2 == 0, edge[k], edge[k + 1]).astype(np.int32)
            exp = s.outcome(want)
            assert (exp["status"][want != srcs] == U.DELIVERED).all()
            U.equal(_query(eng, "device", [want]), exp, "null, nodes %d / %d" % (edge[k], edge[k + 1]))
            U.equal(_query(eng, "host", [want]), exp, "null, host form")
        _both_forms(eng, [s], "null, pick rule")
        got = eng.result_copy(len(srcs), cap=1 << 20)                                # the answers equal a search over these arrays
        np.testing.assert_array_equal(got.dst, s.dst)
        assert (srcs != 1024).all()
        link = _query(eng, "host", [np.full(len(srcs), 1024, dtype=np.int32)])["link"]
        np.testing.assert_array_equal(got.dst[link], 1024)
        np.testing.assert_array_equal(link, got.pkt_offset[:-1] + 1024 - (srcs < 1024))
    finally:
        d.free()
        eng.close()


# ---- 6. batches of both SINR kinds --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("em", [False, True], ids=["plain", "E10"])
@pytest.mark.parametrize("overlap", [False, True], ids=["self-contained", "overlap"])
def test_batches_of_both_kinds(rsa, O, overlap, em):
    nd, lists, starts, air, slots = _batch_ref(overlap, R.SEED if em else None)
    assert any(len(l) == 0 for l in lists) and any((l < 0).any() for l in lists) and max(s.count for s in slots) > 16384
    eng, dev = _engine(rsa, nd, stats=False, em_seed=R.SEED if em else None), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        assert eng.air_batch_stats()[0] == (1 if overlap else 0)
        exp = _both_forms(eng, slots, "batch")
        c = U.counts(exp["status"])
        assert c[U.NOT_SENT] == 3 and min(c[U.UNHEARD], c[U.INTERFERED], c[U.DELIVERED]) >= 8
        # n_pkt smaller than, equal to and larger than a slot's packets: the surplus entries are NONE
        want = U.wants(slots)
        odd = [want[0][:17], np.ones(5, dtype=np.int32), np.concatenate([want[2], np.full(9, 3, dtype=np.int32)]), want[3],
               np.zeros(0, dtype=np.int32), np.concatenate([want[5], want[5]])]
        exp = _expected(slots, odd)
        assert (exp["status"][17:22] == U.NONE).all() and (exp["status"][-len(want[5]):] == U.NONE).all()
        U.equal(_query(eng, "device", odd), exp, "n_pkt smaller / equal / larger")
        U.equal(_query(eng, "host", [np.where(w >= nd.n, -1, w) for w in odd]), _expected(slots, [np.where(w >= nd.n, -1, w) for w in odd]),
                "n_pkt smaller / equal / larger, host form")
        # entry counts around a wave: prefixes of the flat query, over fewer slots
        flat = np.concatenate(want)
        edges = np.cumsum([0] + [len(w) for w in want])
        for n in (1, 63, 64, 65, 130):
            part = [flat[edges[b]:min(edges[b + 1], n)] for b in range(len(want)) if edges[b] < n]
            U.equal(_query(eng, "device", part), _expected(slots, part), "%d entries" % n)
        # every output pointer NULL in turn
        for drop in U.FIELDS:
            keep = tuple(f for f in U.FIELDS if f != drop)
            U.equal(_query(eng, "device", want, fields=keep), _expected(slots, want), "without " + drop, fields=keep)
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 7. the gates: deferred candidates are NOT_SENT ----------------------------------------------------------------------------

def _gated_slots(sc, r, first, last):
    return [U.Slot(sc.nd.n, np.where(r.flags[k] != 0, -1, r.lists[k]), r.exp[k]) for k in range(first, last)]


def test_gated_tick_and_gated_batch(rsa, O):
    sc, r = BR.scene(O, "multi"), BR.run(O, "multi", 12)
    eng = _engine(rsa, sc.nd, sc.params, stats=False)
    try:
        deferred = 0
        for k in range(2):   # E6: two lone gated ticks
            t0, tc, ts = sc.times(k)
            eng.tick_run_sources_cca(t0, t0 + CR.TICK, r.lists[k], ts, CR.AIR, tc, sc.threshold)
            exp = _both_forms(eng, _gated_slots(sc, r, k, k + 1), "gated tick %d" % k)
            deferred += int((exp["status"] == U.NOT_SENT).sum())
        _gated_batch(eng, sc, r.lists[2:12], 2, "device", sc.threshold)   # E7: the rest as one gated batch
        exp = _both_forms(eng, _gated_slots(sc, r, 2, 12), "gated batch")
        deferred += int((exp["status"] == U.NOT_SENT).sum())
        assert deferred > 0 and (exp["status"] == U.DELIVERED).sum() > 0
    finally:
        eng.close()


# ---- 8. CSMA-CA: the at-form over the result's tick / pkt columns, whole and split -------------------------------------------

def _csma_ref(O):
    """csma_ref's `multi`: per tick its Slot and wanted list (pick rule), per packet of the whole its wanted node and expected outcome"""
    def make():
        sc, r = BR.scene(O, "multi"), SR.run(O, "multi")
        slots = [U.Slot(sc.nd.n, r.kept[T], r.exp[T]) for T in range(len(r.lists))]
        want_slots = U.wants(slots)
        outs = [s.outcome(w) for s, w in zip(slots, want_slots)]
        n = len(r.status)
        want = np.full(n, 5, dtype=np.int32)          # (an unsent packet asks for node 5: NONE comes from its tick / pkt of -1)
        exp = U.empty(n)
        for o in np.flatnonzero(r.status == SR.SENT):
            T, i = int(r.tick[o]), int(r.pkt[o])
            want[o] = want_slots[T][i]
            for f in U.FIELDS:
                exp[f][o] = outs[T][f][i]
        return sc, r, want, exp
    return _ref("csma", make)


def test_csma_at_form(rsa, O):
    sc, r, want, exp = _csma_ref(O)
    sent = r.status == SR.SENT
    assert (exp["status"][~sent] == U.NONE).all() and (~sent).sum() > 10
    c = U.counts(exp["status"][sent])
    assert c[U.NONE] > 0 and min(c[U.UNHEARD], c[U.INTERFERED], c[U.DELIVERED]) >= 8
    eng = _engine(rsa, sc.nd, sc.params, stats=False)
    try:
        out, _ = _csma(rsa, eng, sc, r.lists, 0, "device", sc.threshold, SR.SCENES["multi"][1])
        np.testing.assert_array_equal(out["tick"][sent], r.tick[sent])
        np.testing.assert_array_equal(out["pkt"][sent], r.pkt[sent])
        U.equal(_query_at(eng, "device", out["tick"], out["pkt"], want), exp, "CSMA-CA, device form")
        host_want = np.where(want >= sc.nd.n, -1, want)
        exp_h = {f: np.where(host_want < 0, U.empty(len(want))[f], exp[f]) for f in U.FIELDS}
        U.equal(_query_at(eng, "host", out["tick"], out["pkt"], host_want), exp_h, "CSMA-CA, host form")
    finally:
        eng.close()


def test_csma_split_gives_the_same_outcomes(rsa, O):
    """the E9 split of the run at tick 6: every packet's entry from the part in which it was sent equals the whole's"""
    sc, r, want, exp = _csma_ref(O)
    p = SR.SCENES["multi"][1]
    t_cca = [sc.times(k)[1] for k in range(len(r.lists))]
    eng = _engine(rsa, sc.nd, sc.params, stats=False)
    try:
        got = U.empty(len(want))
        carry, ids, done, seen = None, [], 0, np.zeros(len(want), dtype=bool)
        for first, last in ((0, 6), (6, 12)):
            lists = r.lists[first:last]
            out, carried, _, nxt = _part(rsa, eng, sc, lists, first, "device", sc.threshold, p, carry)
            n_own = sum(len(s) for s in lists)
            who = list(ids) + list(range(done, done + n_own))              # the whole's packet of every entry: carried, then own
            slot = np.concatenate([carried["tick"], out["tick"]])
            pkt = np.concatenate([carried["pkt"], out["pkt"]])
            status = np.concatenate([carried["status"], out["status"]])
            ans = _query_at(eng, "device", slot, pkt, want[who])          # before the next evaluating call
            pending = status == SR.PENDING                                # their tick lies behind the part: no such slot
            assert (ans["status"][pending] == U.NONE).all() and (slot[pending] >= last - first).all()
            for e in np.flatnonzero(status == SR.SENT):
                assert not seen[who[e]]
                seen[who[e]] = True
                for f in U.FIELDS:
                    got[f][who[e]] = ans[f][e]
            _, named = KR.collect(lists, t_cca[first:last], carry if carry is not None else [], out, carried)
            ids = [ids[i] if kind == "c" else done + i for kind, i in named]
            done += n_own
            carry = nxt
        np.testing.assert_array_equal(seen, r.status == SR.SENT)
        n6 = sum(len(s) for s in r.lists[:6])
        assert (seen[:n6] & (r.tick[:n6] >= 6)).any()   # packets sent after being carried over the cut
        U.equal(got, exp, "whole against parts", link=False)
    finally:
        eng.close()


# ---- 9. a slot over the link capacity ------------------------------------------------------------------------------------------

def test_a_slot_over_the_link_capacity_is_lost(rsa, O):
    nd, lists, starts, air = R.scene_batch(False)
    lists, starts = [lists[3], lists[4][:3], lists[5][:2]], starts[3:]
    slots = U.sinr_slots(nd, lists, starts, air)
    cap = slots[0].count - 1
    assert cap > 16384 and all(0 < 16 * s.count < cap for s in slots[1:])
    eng, dev = _engine(rsa, nd, stats=False, cap=cap), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        assert [bool(eng.batch_result_count(k)[1]) for k in range(3)] == [True, False, False]
        exp = _both_forms(eng, slots, "one dropped slot", lost=(0,))
        n0 = len(lists[0])
        want0 = U.wants(slots)[0]
        np.testing.assert_array_equal(exp["status"][:n0], np.where(want0 >= 0, U.LOST, U.NONE))
        assert (exp["link"][:n0] == -1).all() and np.isnan(exp["rssi"][:n0]).all() and (exp["reply_src"][:n0] == -1).all()
        assert (exp["link"][n0:] >= 0).any()                                       # the other slots answer normally
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 10. the acknowledgement round trip in lone ticks ---------------------------------------------------------------------------

def test_acknowledgement_round_trip(rsa, O):
    nd, srcs, _, _ = R.scene_lone()
    data, want, d_exp, ack, a_want, a_exp = _ref("ack", lambda: U.ack_round_trip(nd, srcs, R.SEED))
    assert (d_exp["reply_src"] < 0).sum() >= len(srcs) // 4 and (a_exp["status"] == U.DELIVERED).sum() >= 8
    eng = _engine(rsa, nd, stats=False, em_seed=R.SEED)
    d_s, d_w, d_a, out, out2 = DeviceArray(srcs), DeviceArray(want), DeviceArray(a_want), _DevOut(len(srcs)), _DevOut(len(srcs))
    try:
        eng.tick_run_sources_device(0, TICK, d_s.ptr.value, len(srcs), 0, 4064)
        eng.unicast_query_device([len(srcs)], d_w.ptr.value, out.ptrs())
        # the reply list as it lies in device memory is the acknowledgement tick's source list (nothing waited for in between)
        eng.tick_run_sources_device(4256, 4256 + TICK, out.ptrs()["reply_src"], len(srcs), 4256, 352)
        eng.unicast_query_device([len(srcs)], d_a.ptr.value, out2.ptrs())
        eng.sync()
        U.equal(out.read(), d_exp, "data tick")
        U.equal(out2.read(), a_exp, "acknowledgement tick")
    finally:
        for x in (d_s, d_w, d_a, out, out2):
            x.free()
        eng.close()


# ---- 11. the query only reads ---------------------------------------------------------------------------------------------------

def test_query_changes_nothing(rsa, O):
    nd, lists, starts, air, slots = _batch_ref(True, R.SEED)
    eng, dev = _engine(rsa, nd, stats=True, em_seed=R.SEED), []
    probe = np.unique(np.concatenate([l[l >= 0] for l in lists]))[:200].astype(np.int32)
    t_probe = starts[-1] + 1

    def state():
        res = [eng.batch_result_copy(k, len(lists[k]), cap=1 << 20) for k in range(len(lists))]
        cols = [(r.count, r.dst.tobytes(), r.verdict.tobytes(), r.rssi.tobytes(), r.sinr.tobytes(), r.pkt_offset.tobytes(),
                 r.pkt_interference.tobytes()) for r in res]
        energy = eng.channel_energy(t_probe, nodes=probe, cca_threshold_dbm=-90.0)
        tbl, tot = eng.stats_read()
        return cols, energy[0].tobytes(), energy[1].tobytes(), eng.air_batch_stats(), eng.rng_state, tbl.tobytes(), tot

    try:
        eng.seed(5)
        _run_batch(eng, lists, starts, air, dev)
        before = state()
        _both_forms(eng, slots, "with statistics on")
        want = U.wants(slots, host=True)
        slot = np.concatenate([np.full(len(w), b, dtype=np.int32) for b, w in enumerate(want)])
        pkt = np.concatenate([np.arange(len(w), dtype=np.int32) for w in want])
        U.equal(_query_at(eng, "device", slot, pkt, np.concatenate(want)), _expected(slots, want), "at-form over the batch")
        assert state() == before
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 12. refusals: nothing launched, the outputs unwritten -----------------------------------------------------------------------

def test_refusals(rsa, O):
    import ctypes as C
    from radio_sim_amd import _lib
    L = _lib.lib()
    nd, lists, starts, air, slots = _batch_ref(False)
    eng, dev = _engine(rsa, nd, stats=False), []
    n = 8
    want = np.zeros(n, dtype=np.int32)
    d_w, out = DeviceArray(want), _DevOut(n)
    host = {f: np.full(n, SENTINEL[f], dtype=TYPES[f]) for f in U.FIELDS}
    h_out = _lib.UnicastOut(**{f: a.ctypes.data for f, a in host.items()})
    d_out = _lib.UnicastOut(**out.ptrs())
    n_pkt = np.array([n], dtype=np.int32)

    def dev_q(n_slots=1, counts=n_pkt, w=d_w.ptr.value, o=C.byref(d_out)):
        return L.rm_unicast_query_device(eng._h, n_slots, counts.ctypes.data if counts is not None else None, w, o)

    def host_q(w=want, n_slots=1, counts=n_pkt):
        return L.rm_unicast_query(eng._h, n_slots, counts.ctypes.data, w.ctypes.data, C.byref(h_out))

    def at_dev(k=n, s=d_w.ptr.value, p=d_w.ptr.value, w=d_w.ptr.value, o=C.byref(d_out)):
        return L.rm_unicast_query_at_device(eng._h, k, s, p, w, o)

    def at_host(w=want, k=n):
        return L.rm_unicast_query_at(eng._h, k, want.ctypes.data, want.ctypes.data, w.ctypes.data, C.byref(h_out))

    def every(code, what):
        got = [dev_q(), host_q(), at_dev(), at_host()]
        assert got == [code] * 4, (what, got)
        assert len(L.rm_last_error()) > 0

    try:
        every(STATE, "no evaluated result yet")
        _run_batch(eng, lists, starts, air, dev)
        h_before = {f: a.copy() for f, a in host.items()}
        # RM_ERR_INVALID: NULL arguments, counts, n_slots outside 1 .. slots of the last call, a wanted node of a host list
        assert dev_q(o=None) == INVALID and dev_q(w=None) == INVALID and dev_q(counts=None) == INVALID
        assert L.rm_unicast_query_device(None, 1, n_pkt.ctypes.data, d_w.ptr.value, C.byref(d_out)) == INVALID
        assert at_dev(o=None) == INVALID and at_dev(s=None) == INVALID and at_dev(p=None) == INVALID and at_dev(w=None) == INVALID
        assert at_dev(k=-1) == INVALID and at_host(k=-1) == INVALID
        assert L.rm_unicast_query(eng._h, 1, n_pkt.ctypes.data, None, C.byref(h_out)) == INVALID
        assert L.rm_unicast_query(eng._h, 1, n_pkt.ctypes.data, want.ctypes.data, None) == INVALID
        for n_slots in (0, -1, len(lists) + 1, 513):
            assert dev_q(n_slots=n_slots, counts=np.zeros(520, dtype=np.int32)) == INVALID, n_slots
            assert host_q(n_slots=n_slots, counts=np.zeros(520, dtype=np.int32)) == INVALID, n_slots
        neg = np.array([3, -1], dtype=np.int32)
        assert dev_q(n_slots=2, counts=neg) == INVALID and host_q(n_slots=2, counts=neg) == INVALID
        for bad in (nd.n, nd.n + 5):
            w = want.copy()
            w[5] = bad
            assert host_q(w=w) == INVALID and at_host(w=w) == INVALID
        # RM_ERR_CAPACITY: more than 2^27 entries
        big = np.array([2 ** 27, 1], dtype=np.int32)
        assert dev_q(n_slots=2, counts=big) == CAPACITY and host_q(n_slots=2, counts=big) == CAPACITY
        assert at_dev(k=2 ** 27 + 1) == CAPACITY
        # RM_ERR_STATE: a receiver partition; a gathered / rm_dist_* form
        eng.set_partition(0, nd.n // 2)
        every(STATE, "an index partition")
        eng.set_partition_spatial(0, 2)
        every(STATE, "a spatial partition")
        eng.set_partition(0, nd.n)
        src = DeviceArray(lists[0])
        dev.append(src)
        t = 100 * TICK
        eng.batch_run_gathered_sources_device([t], [t + TICK], src.ptr.value, 1, len(lists[0]), [t], air)
        every(STATE, "gathered sources")
        eng.dist_batch_run_sources_device([t + 10 * TICK], [t + 11 * TICK], src.ptr.value, len(lists[0]), [t + 10 * TICK], air)
        every(STATE, "rm_dist_batch")
        eng.dist_tick_run_sources_device(t + 20 * TICK, t + 21 * TICK, src.ptr.value, len(lists[0]), t + 20 * TICK, air)
        every(STATE, "rm_dist_tick")
        eng.sync()
        out.read(written=False)                                                   # no refusal wrote anything
        for f, a in host.items():
            assert a.tobytes() == h_before[f].tobytes(), f
        # a plain tick afterwards is answered again
        eng.tick_run_sources_device(t + 40 * TICK, t + 41 * TICK, src.ptr.value, len(lists[0]), t + 40 * TICK, air)
        assert dev_q(n_slots=2, counts=np.array([1, 1], dtype=np.int32)) == INVALID   # (one slot now)
        assert dev_q() == 0 and host_q() == 0 and at_dev() == 0 and at_host() == 0      # accepted: the sentinels go
        got = out.read()
        assert (got["status"] != SENTINEL["status"]).all() and (host["status"] != SENTINEL["status"]).all()
        np.testing.assert_array_equal(got["status"], host["status"])
        # rm_group_*: a member's results after the group's tick
        grp = rsa.Group([0])
        try:
            grp.upload_table(nd)
            grp.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
            grp.tick(to_tx_records(rsa, nd.packets(lists[0], 0, air)), 0, TICK, cap=1 << 20)
            member = L.rm_group_context(grp._h, 0)
            assert L.rm_unicast_query_device(member, 1, n_pkt.ctypes.data, d_w.ptr.value, C.byref(d_out)) == STATE
        finally:
            grp.close()
    finally:
        d_w.free()
        out.free()
        for d in dev:
            d.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import radio_sim_amd as rsa
eng = rsa.Engine(0)
try:
    try:
        eng.unicast_query([np.zeros(4, dtype=np.int32)])
    except rsa.RadioMediumError as e:
        assert e.code == -5 and "RM_GRAPH" in str(e), e
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_query_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs: the query refuses it
    (ahead of every other check: the refusal names the knob)"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)
