"""The five interference paths of the SINR extension (DESIGN.md sections 4.4, 4.5, 4.7; E3 / E4 of section 6) on the scenes of
tests/sinr_edge_ref.py, every tick bit for bit against the oracle: count, pkt, dst, rssi, sinr, verdict, pkt_interference and the
packet offsets.  A refused call fails the test -- there is no fallback to lone ticks -- and rm_profile_kernels tells whether the
kernels a route is meant to reach ran.  After the last call of a scene one more lone tick looks at what was left on the air."""
import os

import numpy as np
import pytest

import sinr_edge_ref as S
from util import KINDS, _PARAM_MAP, DeviceArray, to_tx_records, sinr_lists_forced

pytestmark = pytest.mark.gpu

GROUP = 64          # rm::kGroup: a table of more nodes is kept in spatial order, which the batched kernels need


def _engine(rsa, sc):
    eng = rsa.Engine(0)
    eng.upload_table(sc.nd)
    eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in sc.params.items()})
    return eng


def _same(gpu, cpu, n_new, what):
    assert gpu.count == cpu.count, (what, gpu.count, cpu.count)
    for f in ("pkt", "dst", "rssi", "sinr", "verdict"):
        np.testing.assert_array_equal(getattr(gpu, f), getattr(cpu, f), err_msg="%s: %s" % (what, f))
    np.testing.assert_array_equal(gpu.pkt_interference[:n_new], cpu.pkt_interference, err_msg=what + ": pkt_interference")
    np.testing.assert_array_equal(gpu.pkt_offset, S.offsets(cpu, n_new), err_msg=what + ": pkt_offset")


def _ran(eng, prefix):
    return sorted(k for k in eng.profile_kernels() if k.startswith(prefix))


class Dev:
    """device arrays of one test, freed together"""

    def __init__(self):
        self.all = []

    def __call__(self, a):
        d = DeviceArray(a) if len(a) else DeviceArray(nbytes=64)
        self.all.append(d)
        return d.ptr.value

    def free(self):
        for d in self.all:
            d.free()


def _lone(eng, dev, t_begin, src, start, air):
    eng.tick_run_sources_device(t_begin, t_begin + S.TICK, dev(np.asarray(src, dtype=np.int32)), len(src), start, air)
    return eng.result_copy(len(src))


def _tail(eng, dev, run, t_begin, what):
    """one more lone tick: what the route left on the air is what the oracle has there"""
    new, cpu, _ = run.tail(t_begin)
    _same(_lone(eng, dev, t_begin, run.sc.tail, t_begin, run.sc.tail_air), cpu, len(new), what + ": the tick after")


def _batch_by_sources(eng, dev, ticks):
    tb = [t.t_begin for t in ticks]
    eng.batch_run_sources_device(tb, [t.t_end for t in ticks], [dev(t.src) if len(t) else 0 for t in ticks], [len(t) for t in ticks],
                                 [t.start for t in ticks], [t.air for t in ticks])


def route_lone(rsa, O, name, lists):
    """(a) every tick on its own, named by a source list"""
    sc, run = S.scene(O, name), S.run(O, name)
    eng, dev = _engine(rsa, sc), Dev()
    try:
        for k, t in enumerate(sc.ticks):
            _same(_lone(eng, dev, t.t_begin, t.src, t.start, t.air), run.exp[k], len(t), "%s: lone tick %d" % (name, k))
        _tail(eng, dev, run, sc.end(), name)
        # the tick by scan takes tables in spatial order; RM_SINR_SCAN=0 keeps every tick on the per-receiver lists
        scanned = eng.air_scan_ticks()
        assert (scanned > 0) == (not lists and sc.nd.n > GROUP), (name, scanned)
    finally:
        dev.free()
        eng.close()


def route_records(rsa, O, name):
    """(b) every tick on its own, its frames as records from the host"""
    sc, run = S.scene(O, name), S.run(O, name)
    eng, dev = _engine(rsa, sc), Dev()
    try:
        for k, t in enumerate(sc.ticks):
            eng.tick_begin(t.t_begin, t.t_end)
            if len(t):
                eng.enqueue_records(to_tx_records(rsa, run.new[k]))
            _same(eng.tick_flush_view(), run.exp[k], len(t), "%s: lone tick %d by records" % (name, k))
        _tail(eng, dev, run, sc.end(), name)
    finally:
        dev.free()
        eng.close()


def route_batch(rsa, O, name, lists):
    """(c) the scene's ticks as ONE batch of self-contained ticks by sources.  Sums per receiver (k_exact_batch in acc mode, then
    k_sinr_acc_batch) where the batched kernels apply: a table in spatial order (more than GROUP nodes) and no empty tick; with
    RM_SINR_ACC=0 the same batch through the per-receiver lists (k_sinr_batch)."""
    sc, run = S.scene(O, name), S.run(O, name)
    assert sc.by_sources and sc.contained
    eng, dev = _engine(rsa, sc), Dev()
    try:
        eng.profile_enable(1)
        _batch_by_sources(eng, dev, sc.ticks)
        for k, t in enumerate(sc.ticks):
            _same(eng.batch_result_copy(k, len(t)), run.exp[k], len(t), "%s: batch tick %d" % (name, k))
        batched = sc.nd.n > GROUP and all(len(t) for t in sc.ticks)
        acc, per_list = _ran(eng, "k_sinr_acc_batch"), _ran(eng, "k_sinr_batch")
        assert bool(acc) == (batched and not lists), (name, sorted(eng.profile_kernels()))
        assert bool(per_list) == (batched and lists), (name, sorted(eng.profile_kernels()))
        assert eng.air_batch_stats() == (0, 0)
        _tail(eng, dev, run, sc.end(), name)
    finally:
        dev.free()
        eng.close()


def route_given(rsa, O, name):
    """(d) the scene's ticks as ONE batch of caller-given records: every frame has a time span of its own inside its tick (a tick
    whose frames outlive 1000 us ends with its last frame)"""
    sc, run = S.scene(O, name), S.run(O, name)
    assert sc.contained
    eng, dev = _engine(rsa, sc), Dev()
    try:
        ends = [max(t.t_end, t.latest_end(sc.nd)) for t in sc.ticks]
        eng.batch_run_device([t.t_begin for t in sc.ticks], ends, [dev(to_tx_records(rsa, new)) for new in run.new], [len(t) for t in sc.ticks])
        for k, t in enumerate(sc.ticks):
            _same(eng.batch_result_copy(k, len(t)), run.exp[k], len(t), "%s: tick %d of a batch of records" % (name, k))
        assert eng.air_batch_stats() == (0, 0)
        _tail(eng, dev, run, ends[-1], name)
    finally:
        dev.free()
        eng.close()


SELF_CONTAINED = [f for f in S.FAMILIES if f not in ("spans", "chain")]


@pytest.mark.parametrize("family", SELF_CONTAINED)
@pytest.mark.parametrize("form", ["scan", "lists"])
def test_lone_ticks_by_sources(rsa, O, monkeypatch, family, form):
    if form == "lists":
        monkeypatch.setenv("RM_SINR_SCAN", "0")
    for name in S.FAMILIES[family]:
        route_lone(rsa, O, name, form == "lists" or sinr_lists_forced())


@pytest.mark.parametrize("family", SELF_CONTAINED + ["spans"])
def test_lone_ticks_by_records(rsa, O, family):
    for name in S.FAMILIES[family]:
        route_records(rsa, O, name)


@pytest.mark.parametrize("family", SELF_CONTAINED)
@pytest.mark.parametrize("form", ["sums", "lists"])
def test_batch_of_self_contained_ticks(rsa, O, monkeypatch, family, form):
    if form == "lists":
        monkeypatch.setenv("RM_SINR_ACC", "0")
    for name in S.FAMILIES[family]:
        route_batch(rsa, O, name, form == "lists" or os.environ.get("RM_SINR_ACC") == "0")


@pytest.mark.parametrize("family", SELF_CONTAINED + ["spans"])
def test_batch_of_given_records(rsa, O, family):
    for name in S.FAMILIES[family]:
        route_given(rsa, O, name)


# ---- (e) the chain of overlapping ticks --------------------------------------------------------------------------------------------
OV_KERNELS = ("k_ov_pairs", "k_ov_exact", "k_ov_verdict")


def _chain_batches(rsa, O, cuts):
    sc, run = S.scene(O, "chain"), S.run(O, "chain")
    eng, dev = _engine(rsa, sc), Dev()
    try:
        edges = [0] + list(cuts) + [len(sc.ticks)]
        overlapping = 0
        for lo, hi in zip(edges, edges[1:]):
            eng.profile_enable(1)
            _batch_by_sources(eng, dev, sc.ticks[lo:hi])
            for k in range(lo, hi):
                _same(eng.batch_result_copy(k - lo, len(sc.ticks[k])), run.exp[k], len(sc.ticks[k]), "chain %s: tick %d" % (cuts, k))
            # frames on the air when the batch begins, or a frame of its own that outlives its tick: the overlap form
            if len(run.before[lo]) or not all(t.latest_end(sc.nd) <= t.t_end for t in sc.ticks[lo:hi - 1]):
                overlapping += 1
                for kernel in OV_KERNELS:
                    assert _ran(eng, kernel), (cuts, lo, kernel, sorted(eng.profile_kernels()))
        assert eng.air_batch_stats()[0] == overlapping == len(edges) - 1
        _tail(eng, dev, run, sc.end(), "chain %s" % (cuts,))
    finally:
        dev.free()
        eng.close()


def test_chain_as_one_overlapping_batch(rsa, O):
    _chain_batches(rsa, O, ())


@pytest.mark.parametrize("cut", S.CHAIN_CUTS)
def test_chain_as_two_batches(rsa, O, cut):
    _chain_batches(rsa, O, (cut,))


@pytest.mark.parametrize("form", ["scan", "lists"])
def test_chain_as_lone_ticks(rsa, O, monkeypatch, form):
    if form == "lists":
        monkeypatch.setenv("RM_SINR_SCAN", "0")
    route_lone(rsa, O, "chain", form == "lists" or sinr_lists_forced())
