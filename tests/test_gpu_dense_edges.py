"""The dense tick (rm_dense.hip) on the scenes of tests/dense_edge_ref.py, every tick bit for bit against the
oracle: count, pkt, dst, rssi, sinr, verdict, pkt_interference, the packet offsets and what rm_result_count says.  Where a scene
is meant to take the dense form the test proves it: rm_result_dense succeeds and its lane masks, decoded on the host
(util.DenseMasks), are the oracle's heard sets.  A run whose environment says RM_DENSE_TICK=0 (tools/knob_sweep.sh) never takes
the dense form: it compares the records all the same and leaves the masks out.  A padding slot's Tx-failure flag is not compared:
the oracle knows no such packet (a slot padded by source index carries txprob 0, which the unit disc flags)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import dense_edge_ref as D
from util import KINDS, _PARAM_MAP, DenseMasks, DeviceArray, assert_same, to_tx_records

pytestmark = pytest.mark.gpu

CAP = 1 << 20
ERR_CAPACITY, ERR_STATE = -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _swept():
    return os.environ.get("RM_DENSE_TICK") == "0"


class Env:
    """the knobs the library reads per tick, set for the ticks that follow (monkeypatch in a test, os.environ in a child process)"""

    def __init__(self, monkeypatch=None):
        self.mp, self.swept = monkeypatch, _swept()

    def _set(self, name, value):
        if value is None:
            self.mp.delenv(name, raising=False) if self.mp else os.environ.pop(name, None)
        else:
            self.mp.setenv(name, value) if self.mp else os.environ.__setitem__(name, value)

    def dense(self, value):
        """"1": whenever the configuration allows it, "0": never, None: the engine's own choice (a swept run keeps its 0)"""
        if not self.swept:
            self._set("RM_DENSE_TICK", value)

    def lazy(self, lazy):
        self._set("RM_DENSE_LAZY", None if lazy else "0")


class Dev:
    """device arrays of one test, freed together"""

    def __init__(self):
        self.all = []

    def __call__(self, a):
        d = DeviceArray(a)
        self.all.append(d)
        return d.ptr.value

    def free(self):
        for d in self.all:
            d.free()


def _same(gpu, exp, what):
    g = types.SimpleNamespace(**{f: getattr(gpu, f) for f in ("count", "pkt", "dst", "verdict", "rssi", "sinr")})
    g.pkt_interference = np.where(exp.real, gpu.pkt_interference, 0).astype(np.uint8)
    assert_same(g, exp, what)
    np.testing.assert_array_equal(gpu.pkt_offset, exp.pkt_offset, err_msg=what + " pkt_offset")


def _masks(eng, sc, tk, exp, what):
    """the tick took the dense form, and its masks are the oracle's heard sets"""
    m = DenseMasks(eng, len(tk), sc.part[0], sc.part[1])
    np.testing.assert_array_equal(m.heard, exp.heard(len(tk), *sc.part), err_msg=what + " masks")
    np.testing.assert_array_equal(m.pkt_offset, exp.pkt_offset, err_msg=what + " pkt_offset of the masks")
    np.testing.assert_array_equal(m.pkt_interference[exp.real], exp.pkt_interference[exp.real], err_msg=what + " flags of the masks")
    assert m.total == exp.count, (what, m.total, exp.count)


def _configure(eng, sc, partition=False, capacity=CAP):
    eng.upload_table(sc.nd)
    eng.set_model(KINDS[sc.kind], **{_PARAM_MAP[k]: v for k, v in sc.params.items()})
    if sc.matrix is not None:
        eng.set_n2n_matrix(sc.matrix)
    if partition:
        eng.set_partition(*sc.part)
    else:
        assert sc.part == (0, sc.nd.n)
    if capacity is not None:
        eng.set_link_capacity(capacity)


def _by_sources(eng, dev, tk):
    eng.tick_run_sources_device(tk.t_begin, tk.t_end, dev(tk.src), len(tk), tk.start, tk.air)


def run_scene(rsa, O, eng, dev, env, name, partition=False):
    """one scene through the three ways a tick's frames reach the engine"""
    sc = D.scene(O, name)
    env.dense("1" if sc.force else None)
    _configure(eng, sc, partition)
    dense = bool(sc.dense) and not env.swept
    for k, tk in enumerate(sc.ticks):
        exp = D.expected(O, name, k)
        recs = to_tx_records(rsa, tk.packets(sc.nd))
        cap = exp.count + 4096
        # (a) records from the host
        _same(eng.tick(recs, tk.t_begin, tk.t_end, cap=cap), exp, name + ": host records")
        if dense:
            _masks(eng, sc, tk, exp, name + ": host records")
        # (b) source indices on the device: the totals first (they do not wait for the records), the masks, then the records
        _by_sources(eng, dev, tk)
        assert eng.result_count() == (exp.count, 0), name
        if dense:
            _masks(eng, sc, tk, exp, name + ": source indices")
        _same(eng.result_copy(len(tk), cap=cap), exp, name + ": source indices on the device")
        # (c) the caller's records in device memory: the records first, the masks outlive them
        eng.tick_run_device(tk.t_begin, tk.t_end, dev(recs), len(tk))
        _same(eng.result_copy(len(tk), cap=cap), exp, name + ": the caller's device records")
        if dense:
            _masks(eng, sc, tk, exp, name + ": the caller's device records")
        assert eng.result_count() == (exp.count, 0), name


# ---- 1. every scene ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lazy", "at-once"])
@pytest.mark.parametrize("family", list(D.FAMILIES))
def test_every_scene_by_host_records_source_indices_and_device_records(rsa, O, monkeypatch, family, mode):
    """both record modes: the records on request (the tick ends with its cells) and RM_DENSE_LAZY=0 (the records at once: the
    fused write pass up to 8192 cells, the scan beyond)"""
    env = Env(monkeypatch)
    env.lazy(mode == "lazy")
    eng, dev = rsa.Engine(0), Dev()
    try:
        for name in D.FAMILIES[family]:
            run_scene(rsa, O, eng, dev, env, name, partition=(family == "parts"))
    finally:
        dev.free()
        eng.close()


def test_lattice3d_edge_pairs_through_the_culled_kernels(rsa, O, monkeypatch):
    """RM_DENSE_TICK=0: the same pairs at d == range through eval_link"""
    monkeypatch.setenv("RM_DENSE_TICK", "0")
    eng, dev = rsa.Engine(0), Dev()
    try:
        for name in D.FAMILIES["lattice3d"]:
            sc, exp = D.scene(O, name), D.expected(O, name)
            tk = sc.ticks[0]
            _configure(eng, sc)
            _same(eng.tick(to_tx_records(rsa, tk.packets(sc.nd)), cap=exp.count + 4096), exp, name + ": culled, host records")
            with pytest.raises(rsa.RadioMediumError):
                eng.result_dense()
            _by_sources(eng, dev, tk)
            _same(eng.result_copy(len(tk), cap=exp.count + 4096), exp, name + ": culled, source indices")
    finally:
        dev.free()
        eng.close()


# ---- 2. what a dense tick leaves for the tick that follows ------------------------------------------------------------------------------
# (scene, the knob, records at once?, what is read of the result)
TAILS = [
    ("cells/8190", "1", True, "records"),             # the fused write pass runs the tail (<= 8192 cells)
    ("culled/udgm/0", "0", True, "records"),
    ("cells/8195", "1", True, "records"),             # the scan runs the tail (its loop: more than 8192 cells)
    ("culled/logdist/0", None, True, "records"),
    ("cells/small/0", "1", False, "count"),           # the count pass runs the tail; only the totals are read
    ("culled/udgm/1", "0", False, "records"),
    ("cells/small/2", "1", False, "nothing"),         # ... and nobody reads anything
    ("culled/logdist/1", None, False, "records"),
    ("cells/8195", "1", False, "records"),
    ("cells/small/1", "1", False, "records"),         # 9 frames after 1639: the per-frame arrays shrink
    ("culled/udgm/0", "0", False, "records"),
    ("cells/8195", "1", True, "records"),
    ("cells/small/1", "1", True, "records"),          # the same with the records at once
    ("cells/small/3", "1", True, "records"),          # 64 frames: 320 cells through the fused pass after the scan
    ("culled/logdist/0", None, True, "records"),
]


def tails_sequence(rsa, O, env):
    """dense and culled ticks one after the other on ONE context, each against the oracle: every kernel that runs
    dense_tick_tail is followed by a culled tick"""
    eng, dev = rsa.Engine(0), Dev()
    try:
        eng.upload_table(D.cells_table(O, 5000))
        eng.set_link_capacity(CAP)
        model = None
        for step, (name, knob, at_once, read) in enumerate(TAILS):
            sc, exp = D.scene(O, name), D.expected(O, name)
            tk, what = sc.ticks[0], "step %d (%s)" % (step, name)
            if (sc.kind, sc.params) != model:
                eng.set_model(KINDS[sc.kind], **{_PARAM_MAP[k]: v for k, v in sc.params.items()})
                model = (sc.kind, sc.params)
            env.dense(knob)
            env.lazy(not at_once)
            t0 = step * D.TICK
            eng.tick_run_sources_device(t0, t0 + D.TICK, dev(tk.src), len(tk), t0, tk.air)
            if read == "nothing":
                continue
            assert eng.result_count() == (exp.count, 0), what
            if read == "count":
                continue
            _same(eng.result_copy(len(tk), cap=exp.count + 4096), exp, what)
            if sc.dense and not env.swept:
                _masks(eng, sc, tk, exp, what)
            elif not sc.dense:
                with pytest.raises(rsa.RadioMediumError):
                    eng.result_dense()
    finally:
        dev.free()
        eng.close()


def test_tails_dense_and_culled_ticks_alternate_on_one_context(rsa, O, monkeypatch):
    tails_sequence(rsa, O, Env(monkeypatch))


def test_tails_with_the_culled_ticks_in_three_launches(O):
    """RM_FRAME_TICK=0 is read once per process: the same sequence in a child of its own (the culled ticks then run the filter,
    exact and reorder kernels, whose counters the dense tick's tail has to leave as the sweep's first kernel would)"""
    for name, _, _, _ in TAILS:
        D.expected(O, name)          # (a scene that cannot be built fails here, not in the child)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "tails"], env=dict(os.environ, RM_FRAME_TICK="0"), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert r.returncode == 0, r.stdout.decode("utf-8", "replace")[-4000:]


# ---- 3. capacity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lazy", "at-once"])
@pytest.mark.parametrize("name", ["lattice3d/udgm7", "cells/8195"])
def test_link_capacity_of_exactly_the_total_and_of_one_less(rsa, O, monkeypatch, name, mode):
    """cap == total: no drop, every record; cap == total - 1: RM_ERR_CAPACITY, and rm_result_count says (total, dropped) -- on
    both sides of 8192 cells (300 and 8195), in both record modes (the record pass's o < cap guard drops the last record)"""
    env = Env(monkeypatch)
    env.lazy(mode == "lazy")
    sc, exp = D.scene(O, name), D.expected(O, name)
    tk, total = sc.ticks[0], exp.count
    env.dense("1" if sc.force else None)
    eng, dev = rsa.Engine(0), Dev()
    try:
        _configure(eng, sc)
        recs = to_tx_records(rsa, tk.packets(sc.nd))
        for cap in (total, total - 1, total):
            eng.set_link_capacity(cap)
            _by_sources(eng, dev, tk)
            assert eng.result_count() == (total, 0 if cap == total else 1), (name, cap)
            if cap == total:
                _same(eng.result_copy(len(tk), cap=total + 4096), exp, "%s: capacity %d" % (name, cap))
                if not env.swept:
                    _masks(eng, sc, tk, exp, name)
                _same(eng.tick(recs, cap=total + 4096), exp, "%s: capacity %d, host records" % (name, cap))
            else:
                with pytest.raises(rsa.RadioMediumError) as e:
                    eng.result_copy(len(tk), cap=total + 4096)
                assert e.value.code == ERR_CAPACITY
                with pytest.raises(rsa.RadioMediumError) as e:
                    eng.tick(recs, cap=total + 4096)
                assert e.value.code == ERR_CAPACITY
    finally:
        dev.free()
        eng.close()


# ---- 4. the records are written when somebody asks -----------------------------------------------------------------------------------
def test_lazy_records_are_the_ticks_own_after_later_node_updates(rsa, O, monkeypatch):
    """A lazy dense tick, then rm_node_update -- a heard receiver moved out of range, another switched off, a source's power
    changed -- and only then the first rm_result_copy.  The masks, the flags and the frames' records were left by the tick itself,
    and a result is valid until the next evaluating call (radiomedium_hip.h): the records are the tick-time oracle's.  A refusal
    with RM_ERR_STATE would be the one other honest answer; anything else -- records of the changed table -- fails."""
    env = Env(monkeypatch)
    env.lazy(True)
    name = "lattice3d/udgm7"
    sc, exp = D.scene(O, name), D.expected(O, name)
    tk, nd = sc.ticks[0], sc.nd
    eng, dev = rsa.Engine(0), Dev()
    try:
        _configure(eng, sc)
        _by_sources(eng, dev, tk)
        moved, off = int(exp.dst[0]), int(exp.dst[exp.count // 2])
        source = int(tk.src[exp.pkt[exp.count // 3]])
        assert len({moved, off, source}) == 3

        def update(j, **kw):
            v = dict(x=nd.x[j], y=nd.y[j], z=nd.z[j], txpower=nd.txpower[j], channel=int(nd.channel[j]), enabled=int(nd.enabled[j]),
                     rxprob=nd.rxprob[j], txprob=nd.txprob[j])
            v.update(kw)
            eng.update_node(j, v["x"], v["y"], v["z"], v["txpower"], v["channel"], v["enabled"], v["rxprob"], v["txprob"])
        update(moved, x=nd.x[moved] + 1000.0)
        update(off, enabled=0)
        update(source, txpower=nd.txpower[source] + 3.0)
        try:
            got = eng.result_copy(len(tk), cap=exp.count + 4096)
        except rsa.RadioMediumError as e:
            assert e.code == ERR_STATE
        else:
            _same(got, exp, name + ": first read after the node updates")
            if not env.swept:
                _masks(eng, sc, tk, exp, name + ": after the node updates")
        # the next tick sees the changed table (the oracle's, with the same three changes)
        nd2 = O.NodeTable(nd.n)
        for f in ("x", "y", "z", "txpower", "channel", "enabled", "rxprob", "txprob", "int_id"):
            setattr(nd2, f, getattr(nd, f).copy())
        nd2.x[moved] += 1000.0
        nd2.enabled[off] = 0
        nd2.txpower[source] += 3.0
        after = D.Expected(O, D.Scene(name + "/after", nd2, sc.kind, sc.params, sc.ticks, force=False), tk)
        assert after.count < exp.count
        _by_sources(eng, dev, tk)
        _same(eng.result_copy(len(tk), cap=exp.count + 4096), after, name + ": the tick after the node updates")
    finally:
        dev.free()
        eng.close()


# ---- 5. a batch of Null-medium ticks ---------------------------------------------------------------------------------------------------
def test_batch_of_null_medium_ticks_read_in_reverse(rsa, O, monkeypatch):
    """the Null medium's table is not in spatial order, so the batch runs its ticks one by one and every slot is a dense tick
    of its own: 3, 8, 9, 1 and 17 frames on 2049 nodes, the results read from the last slot to the first"""
    env = Env(monkeypatch)
    env.lazy(True)
    env.dense(None)
    nd = D.shape_table(O, 2049)
    ticks = [D.Tick(D._sources(2049, t, 300 + t), k) for k, t in enumerate((3, 8, 9, 1, 17))]
    sc = D.Scene("batch/null", nd, "null", {}, ticks, force=False)
    exps = [D.Expected(O, sc, tk) for tk in ticks]
    eng, dev = rsa.Engine(0), Dev()
    try:
        _configure(eng, sc)
        eng.batch_run_sources_device([t.t_begin for t in ticks], [t.t_end for t in ticks], [dev(t.src) for t in ticks], [len(t) for t in ticks],
                                     [t.start for t in ticks], [t.air for t in ticks])
        for k in reversed(range(len(ticks))):
            assert eng.batch_result_count(k) == (exps[k].count, 0), k
            _same(eng.batch_result_copy(k, len(ticks[k]), cap=exps[k].count + 4096), exps[k], "batch slot %d" % k)
        for k in range(len(ticks)):      # ... and once more, forwards: a slot's records are written once and stay
            _same(eng.batch_result_copy(k, len(ticks[k]), cap=exps[k].count + 4096), exps[k], "batch slot %d again" % k)
    finally:
        dev.free()
        eng.close()


# ---- 6. the 0/1 matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knob", [None, "1"])
def test_n2n_matrix_of_zeros_and_ones(rsa, O, monkeypatch, knob):
    """whichever form the tick takes -- the test does not say -- its records are the oracle's; masks, if handed out, are its sets
    (the context keeps its default link capacity: the general path deals a table's candidates to shards of capacity / 64 links)"""
    env = Env(monkeypatch)
    env.lazy(True)
    sc, exp = D.scene(O, "n2n01"), D.expected(O, "n2n01")
    tk = sc.ticks[0]
    eng, dev = rsa.Engine(0), Dev()
    try:
        _configure(eng, sc, capacity=None)
        env.dense(knob)
        _same(eng.tick(to_tx_records(rsa, tk.packets(sc.nd)), cap=exp.count + 4096), exp, "n2n01: host records")
        _by_sources(eng, dev, tk)
        try:
            eng.result_dense()
        except rsa.RadioMediumError:
            pass
        else:
            _masks(eng, sc, tk, exp, "n2n01")
        _same(eng.result_copy(len(tk), cap=exp.count + 4096), exp, "n2n01: source indices on the device")
    finally:
        dev.free()
        eng.close()


if __name__ == "__main__":      # the child of test_tails_with_the_culled_ticks_in_three_launches
    assert sys.argv[1:] == ["tails"]
    sys.path.insert(0, ROOT)
    import radio_sim_amd
    from oracle import oracle
    oracle.lib()
    tails_sequence(radio_sim_amd, oracle, Env())
    print("tails: %d ticks on one context, every one read is the oracle's" % len(TAILS))
