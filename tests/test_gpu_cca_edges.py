"""The carrier-sense kernels (DESIGN.md sections 4.9 - 4.11: the channel energy query, the lone gate, the gated batch) on the GPU, on
the scenes of tests/cca_edge_ref.py: a hot spot that overflows the index's cells and fills the EVERY list beyond one LDS chunk, sums
that use the high word, a tick of more than 1024 candidates, air times that differ per tick with exact span ends, RM_MAX_BATCH mostly
empty ticks, ld_exponent = 0, a node outside the fp32 frame.  tests/test_cca_edge_ref.py holds the scenes to the conditions that make
them reach those branches.  Expected values come from the oracle alone; everything is compared bit for bit: flags, energies, pkt,
dst, verdict, rssi, sinr, pkt_offset, the Tx-failure flags, and the window after the call through rm_channel_energy."""
import types

import numpy as np
import pytest

import cca_edge_ref as ER
import cca_ref as CR
import energy_ref as R
from test_gpu_cca import _engine, _gated, _same_links, _same_sense
from test_gpu_cca import _window_is as _window_at
from test_gpu_cca_batch import _batch, _check_batch, _gated_call, _refused
from test_gpu_energy import _device_query, _same
from util import DeviceArray

pytestmark = pytest.mark.gpu


def _ran(eng):
    return {k for k in eng.profile_kernels() if k.startswith(("k_cca", "k_energy"))}


def _step(eng, sc, r, k, form="device"):
    """step k of the scene on the engine, plain or as a lone gated tick, against the run"""
    t0, tc, ts = sc.times(k)
    src, what = r.lists[k], "%s, step %d" % (sc.name, k)
    if sc.gated[k]:
        _same_sense(_gated(eng, form, t0, src, ts, sc.airs[k], tc, sc.threshold), (r.flags[k], r.energy[k]), what)
    else:
        d = DeviceArray(src)
        try:
            eng.tick_run_sources_device(t0, t0 + CR.TICK, d.ptr.value, len(src), ts, sc.airs[k])
            eng.sync()
        finally:
            d.free()
    _same_links(eng.result_copy(len(src), cap=1 << 22), r.exp[k], what)


def _window(eng, O, sc, r, k, nodes, what):
    """the frames on the air after step k, through the query at the step's start + 1"""
    chain = types.SimpleNamespace(nd=sc.nd, mdl=sc.model(O), onair=r.onair[k])
    _window_at(eng, O, chain, sc.start[k] + 1, np.asarray(nodes, dtype=np.int32), what + ": the window after step %d" % k)


def _batch_steps(eng, sc, r, first, last, form="device"):
    got = _batch(eng, sc, r.lists[first:last], first, form, sc.threshold, air=sc.airs[first:last])
    _check_batch(eng, r, first, last, got, "%s, steps %d .. %d as one batch (%s form)" % (sc.name, first, last - 1, form))
    return got


# ---- 1. hotspot ----------------------------------------------------------------------------------------------------------------------
def _hotspot(rsa, O, upto):
    sc, r = ER.scene(O, "hotspot"), ER.run(O, "hotspot")
    eng = _engine(rsa, sc.nd, sc.params, cap=1 << 22)
    try:
        for k in range(upto):
            _step(eng, sc, r, k)
        eng.profile_enable(1)
    except BaseException:
        eng.close()
        raise
    return sc, r, eng


def test_hotspot_query(rsa, O):
    """1152 live frames in at most 4 cells of 16: the cells overflow, the EVERY list is longer than one chunk of 256; sums above 2^64.
    Own channels and one forced channel, host and device form."""
    sc, r, eng = _hotspot(rsa, O, ER.HOT_QUERY)
    try:
        t, nodes = sc.t_cca[ER.HOT_QUERY], sc.query_nodes
        for channel in (None, 13):
            want = R.channel_energy(O, sc.model(O), sc.nd, r.before[ER.HOT_QUERY], t, nodes=nodes, channel=channel, threshold=sc.threshold)
            _same(eng.channel_energy(t, nodes=nodes, channel=channel, cca_threshold_dbm=sc.threshold), want, "hotspot, host form, channel %s" % channel)
            _same(_device_query(eng, t, len(nodes), nodes=nodes, channel=channel, thr=sc.threshold), want, "hotspot, device form, channel %s" % channel)
        assert _ran(eng) == {"k_energy_index<true>", "k_energy_sum<true>"}, _ran(eng)
        # every node in the receiver table's order (one lane per node, a wave walks the same cells): the listed ones against the oracle
        e, f = eng.channel_energy(t, cca_threshold_dbm=sc.threshold)
        _same((e[nodes], f[nodes]), R.channel_energy(O, sc.model(O), sc.nd, r.before[ER.HOT_QUERY], t, nodes=nodes, threshold=sc.threshold), "hotspot, all nodes")
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_hotspot_lone_gate(rsa, O, form):
    sc, r, eng = _hotspot(rsa, O, ER.HOT_GATE)
    try:
        _step(eng, sc, r, ER.HOT_GATE, form)
        assert _ran(eng) == {"k_energy_index<true>", "k_cca_gate<true>"}, _ran(eng)
        _window(eng, O, sc, r, ER.HOT_GATE, np.concatenate([r.lists[ER.HOT_GATE], sc.query_nodes[:60]]), "hotspot")
    finally:
        eng.close()


@pytest.mark.parametrize("split", [(6,), (2, 4)], ids=["one-batch", "2+4"])
def test_hotspot_gated_batch(rsa, O, split):
    """The batch's cells hold 64: 1152 window frames and some 400 candidates in at most 4 cells overflow them.  As one batch and as 2 + 4:
    both equal the oracle's chain, hence each other."""
    sc, r, eng = _hotspot(rsa, O, ER.HOT_BATCH[0])
    try:
        k = ER.HOT_BATCH[0]
        for size in split:
            _batch_steps(eng, sc, r, k, k + size, "device" if size != 2 else "host")
            k += size
            _window(eng, O, sc, r, k - 1, np.concatenate([r.lists[k - 1], sc.query_nodes[:60]]), "hotspot")
        assert k == ER.HOT_BATCH[1]
        assert {"k_ccab_index<true>", "k_ccab_pairs<true, false>", "k_ccab_pairs<true, true>", "k_ccab_resolve"} <= _ran(eng), _ran(eng)
        assert not {"k_ccab_index<false>", "k_ccab_pairs<false, false>", "k_ccab_pairs<false, true>"} & _ran(eng), _ran(eng)
    finally:
        eng.close()


# ---- 2. bigtick ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_bigtick(rsa, O, form):
    """One batch of overlapping ticks with 1300, 40, 1100 and 40 candidates: the one resolving workgroup of 1024 threads strides over
    a tick, the short ticks read kept bits of slots >= 1024, and 2480 candidates are three workgroups of the scan."""
    sc, r = ER.scene(O, "bigtick"), ER.run(O, "bigtick")
    eng = _engine(rsa, sc.nd, sc.params, cap=1 << 22)
    try:
        _step(eng, sc, r, 0)
        eng.profile_enable(1)
        _batch_steps(eng, sc, r, 1, 5, form)
        assert {"k_ccab_index<true>", "k_ccab_scan_top", "k_ccab_resolve"} <= _ran(eng), _ran(eng)
        rng = np.random.default_rng(2)
        nodes = np.concatenate([r.lists[2], r.lists[4], r.lists[1][1000:1060], r.lists[3][1000:1060], rng.integers(0, sc.nd.n, 100)])
        _window(eng, O, sc, r, 4, nodes, "bigtick")
    finally:
        eng.close()


# ---- 3. times ------------------------------------------------------------------------------------------------------------------------
def test_times(rsa, O):
    """Six ticks with an air time each (one of 0), spans that end exactly at a later tick's sample and one microsecond after it, two
    ticks at the same instant with sample == start, a window frame that ends at one sample and one past another: as one batch, and on
    a second context as lone gated ticks."""
    sc, r = ER.scene(O, "times"), ER.run(O, "times")
    n = len(sc.ticks)
    nodes = np.concatenate(r.lists)
    a, b = _engine(rsa, sc.nd, sc.params), _engine(rsa, sc.nd, sc.params)
    try:
        for eng in (a, b):
            _step(eng, sc, r, 0)
        got = _batch_steps(a, sc, r, 1, n)
        _window(a, O, sc, r, n - 1, nodes, "times, one batch")
        for k in range(1, n):
            _step(b, sc, r, k)
        _window(b, O, sc, r, n - 1, nodes, "times, lone gated ticks")
        ea, eb = a.channel_energy(sc.start[n - 1] + 1), b.channel_energy(sc.start[n - 1] + 1)
        _same(ea, eb, "times: the window of the batch against the lone ticks', every node")
        assert got[3][0].size == len(r.lists[4]) and a.batch_result_count(3)[0] == r.exp[4].count          # (the tick whose frames last 0 us)
    finally:
        a.close()
        b.close()


# ---- 4. sparse512 --------------------------------------------------------------------------------------------------------------------
def test_sparse512(rsa, O, form="device"):
    """RM_MAX_BATCH ticks, 21 of them with candidates: the search for a candidate's tick runs over descriptors most of which share an
    offset, and the ticks' start and air times fill the pairs kernel's 512 entries.  (The device form only: the call plans 512 tick
    slots, which takes the engine some four seconds on the host whatever the scene's size.)"""
    sc, r = ER.scene(O, "sparse512"), ER.run(O, "sparse512")
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        got = _batch(eng, sc, r.lists, 0, form, sc.threshold, air=sc.airs)
        for k in sorted(set(ER.SPARSE_FULL) | {0, 2, 8, 57, 107, 204, 510, 511}):        # every tick with candidates, some without
            _same_sense(got[k], (r.flags[k], r.energy[k]), "sparse512, %s form, tick %d" % (form, k))
            _same_links(eng.batch_result_copy(k, len(r.lists[k]), cap=1 << 20), r.exp[k], "sparse512, %s form, tick %d" % (form, k))
        assert sum(len(g[0]) for g in got) == sum(len(s) for s in r.lists)
        _window(eng, O, sc, r, ER.MAX_BATCH - 1, np.concatenate([r.lists[k] for k in ER.SPARSE_FULL[-3:]]), "sparse512")
    finally:
        eng.close()


# ---- 5. flat -------------------------------------------------------------------------------------------------------------------------
def test_flat(rsa, O):
    """ld_exponent = 0: every frame that reaches the floor reaches it everywhere -- with the grid selected by the window's size, all of
    them are in the EVERY list and no cell holds any.  A query, a lone gated tick, a gated batch of three ticks."""
    sc, r = ER.scene(O, "flat"), ER.run(O, "flat")
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        for k in range(ER.FLAT_QUERY):
            _step(eng, sc, r, k)
        eng.profile_enable(1)
        t, nodes = sc.t_cca[ER.FLAT_QUERY], sc.query_nodes
        for channel in (None, 12):
            want = R.channel_energy(O, sc.model(O), sc.nd, r.before[ER.FLAT_QUERY], t, nodes=nodes, channel=channel, threshold=sc.threshold)
            _same(eng.channel_energy(t, nodes=nodes, channel=channel, cca_threshold_dbm=sc.threshold), want, "flat, host form, channel %s" % channel)
            _same(_device_query(eng, t, len(nodes), nodes=nodes, channel=channel, thr=sc.threshold), want, "flat, device form, channel %s" % channel)
        want = R.channel_energy(O, sc.model(O), sc.nd, r.before[ER.FLAT_QUERY], t, threshold=sc.threshold)
        _same(eng.channel_energy(t, cca_threshold_dbm=sc.threshold), want, "flat, all nodes")
        assert _ran(eng) == {"k_energy_index<true>", "k_energy_sum<true>"}, _ran(eng)
        _step(eng, sc, r, ER.FLAT_GATE)
        assert _ran(eng) == {"k_energy_index<true>", "k_energy_sum<true>", "k_cca_gate<true>"}, _ran(eng)
        first, last = ER.FLAT_BATCH
        _batch_steps(eng, sc, r, first, last)
        assert {"k_ccab_index<true>", "k_ccab_pairs<true, false>", "k_ccab_pairs<true, true>"} <= _ran(eng), _ran(eng)
        assert not {"k_energy_index<false>", "k_cca_gate<false>", "k_ccab_index<false>"} & _ran(eng), _ran(eng)
        _window(eng, O, sc, r, last - 1, np.arange(sc.nd.n), "flat")
    finally:
        eng.close()


# ---- 6. a node outside the fp32 frame ------------------------------------------------------------------------------------------------
def test_far_node_in_the_query(rsa, O):
    """One node 3000 km away: fp32 cannot hold the frame's positions, the link-hash table is off.  The query for all nodes and for a
    list with the far node; the gated batch refuses this context with RM_ERR_STATE and leaves the window as it was."""
    from radio_sim_amd import _lib
    from radio_sim_amd import workload as W
    nd, params, srcs, frames, far = ER.far_scene(O)
    mdl = O.model(4, **params)
    eng = _engine(rsa, nd, params)
    try:
        d = DeviceArray(srcs)
        eng.tick_run_sources_device(0, 1000, d.ptr.value, len(srcs), 0, W.AIR_US)
        eng.sync()
        d.free()
        want = R.channel_energy(O, mdl, nd, frames, 500, threshold=-90.0)
        assert want[0][far] == -100.0 and (want[2] >= 4).mean() >= 0.5
        _same(eng.channel_energy(500, cca_threshold_dbm=-90.0), want, "all nodes, host form")
        _same(_device_query(eng, 500, nd.n, thr=-90.0), want, "all nodes, device form")
        rng = np.random.default_rng(9)
        lst = np.concatenate([rng.integers(0, nd.n, 300), [far], srcs[:10], [far]]).astype(np.int32)
        listed = (want[0][lst], want[1][lst])
        _same(eng.channel_energy(500, nodes=lst, cca_threshold_dbm=-90.0), listed, "a list with the far node, host form")
        _same(_device_query(eng, 500, len(lst), nodes=lst, thr=-90.0), listed, "a list with the far node, device form")
        # two overlapping gated ticks: the batched form needs an fp32 frame
        lists = [np.array([far, 5, 6, 7], dtype=np.int32), np.array([8, 9, far], dtype=np.int32)]
        for form in ("host", "device"):
            _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, form, [1000, 2000], [2000, 3000], lists, [1200, 2200], [W.AIR_US] * 2, [1100, 2100]))
            want = R.channel_energy(O, mdl, nd, frames, 1100, threshold=-90.0)
            assert (want[0] > -100.0).any()
            _same(eng.channel_energy(1100, cca_threshold_dbm=-90.0), want, "after the refusal (%s form)" % form)
    finally:
        eng.close()
