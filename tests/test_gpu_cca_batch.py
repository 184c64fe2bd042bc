"""The carrier-sense gated batch (rm_batch_run_sources_cca*) on the GPU.  Expected values come from the oracle
alone: tests/cca_ref.py::Chain.gated_tick called tick by tick is E7's definition (tests/cca_batch_ref.py runs it once per scene and
keeps the result; tests/test_cca_batch_ref.py holds the scenes' conditions).  Everything is compared bit for bit: flags, energies, per
slot count, pkt, dst, verdict, rssi, sinr, pkt_offset and the Tx-failure flags, and the window after the batch through
rm_channel_energy with the candidates among the queried nodes."""
import numpy as np
import pytest

import cca_batch_ref as BR
import cca_ref as CR
import energy_ref as R
from test_gpu_cca import _bits, _engine, _same_links, _same_sense
from util import DeviceArray, KINDS, _PARAM_MAP

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _times(sc, first, last):
    t = [sc.times(k) for k in range(first, last)]
    return [x[0] for x in t], [x[0] + CR.TICK for x in t], [x[1] for x in t], [x[2] for x in t]      # begin, end, sample, start


def _batch(eng, sc, lists, first, form, thr, air=CR.AIR):
    """ticks first .. first+len(lists)-1 of the scene's clock as ONE gated batch -> per tick (flags, energy); the device form through
    device arrays, with the caller's lists checked to be unwritten.  `air`: one air time for every tick, or a list with one per tick"""
    lists = [np.ascontiguousarray(s, dtype=np.int32) for s in lists]
    tb, te, tc, ts = _times(sc, first, first + len(lists))
    airs = list(air) if isinstance(air, (list, tuple)) else [air] * len(lists)
    assert len(airs) == len(lists)
    if form == "host":
        f, e = eng.batch_run_sources_cca(tb, te, lists, ts, airs, tc, thr)
        return list(zip(f, e))
    total = sum(len(s) for s in lists)
    d_s = [DeviceArray(s) if len(s) else None for s in lists]
    d_f = DeviceArray(np.full(max(total, 1), 77, dtype=np.uint8))
    d_e = DeviceArray(np.full(max(total, 1), 12345.0))
    try:
        eng.batch_run_sources_cca_device(tb, te, [d.ptr.value if d else None for d in d_s], [len(s) for s in lists], ts, airs, tc, thr,
                                         d_f.ptr.value, d_e.ptr.value)
        eng.sync()
        for d, s in zip(d_s, lists):
            if d:
                np.testing.assert_array_equal(DeviceArray.read(d.ptr.value, np.int32, len(s)), s, err_msg="a caller's dev_src was written")
        f = DeviceArray.read(d_f.ptr.value, np.uint8, max(total, 1))[:total]
        e = DeviceArray.read(d_e.ptr.value, np.float64, max(total, 1))[:total]
        cuts = np.cumsum([len(s) for s in lists])[:-1]
        return list(zip(np.split(f, cuts), np.split(e, cuts)))
    finally:
        for d in d_s + [d_f, d_e]:
            if d:
                d.free()


def _check_batch(eng, r, first, last, got, what):
    for b, k in enumerate(range(first, last)):
        _same_sense(got[b], (r.flags[k], r.energy[k]), "%s, tick %d" % (what, k))
        _same_links(eng.batch_result_copy(b, len(r.lists[k]), cap=1 << 22), r.exp[k], "%s, tick %d" % (what, k))


def _window_is(eng, O, sc, r, k, what):
    """the frames on the air after tick k, through the query, the batch's candidates among the queried nodes"""
    t = sc.times(k)[2] + 1
    rng = np.random.default_rng(77 + k)
    nodes = np.concatenate(r.lists[max(0, k - 8):k + 1] + [rng.integers(0, sc.nd.n, 100).astype(np.int32)])
    nodes = np.unique(nodes[(nodes >= 0) & (nodes < sc.nd.n)]).astype(np.int32)
    want = R.channel_energy(O, sc.model(O), sc.nd, r.onair[k], t, nodes=nodes, threshold=-90.0)
    got = eng.channel_energy(t, nodes=nodes, cca_threshold_dbm=-90.0)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": window flags")
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=what + ": window energy")


def _kernels(eng):
    return {k for k in eng.profile_kernels() if k.startswith("k_ccab")}


@pytest.mark.parametrize("form", ["device", "host"])
def test_multi_scene_one_batch(rsa, O, form):
    """6000 nodes with shadowing, 12 ticks x 150 candidates (padding on input), frames of 8128 us over ticks of 1000 us: one batch"""
    sc, r = BR.scene(O, "multi"), BR.run(O, "multi", 12)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        got = _batch(eng, sc, r.lists, 0, form, sc.threshold)
        _check_batch(eng, r, 0, 12, got, "multi, %s form" % form)
        _window_is(eng, O, sc, r, 11, "multi, %s form" % form)
    finally:
        eng.close()


def test_split_invariance(rsa, O):
    """The same twelve ticks as one batch, as batches of 5 + 7, and as four lone gated ticks followed by a batch of 8 (which begins
    with 600 records in the window): all three equal the oracle chain, hence each other.  The index takes the grid when the window's
    records plus the batch's candidates reach kEdSmallWindow (256): it does in all three (the list-only form: test_edge_lists)."""
    sc, r = BR.scene(O, "multi"), BR.run(O, "multi", 12)
    for split in ((12,), (5, 7), (1, 1, 1, 1, 8)):
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            eng.profile_enable(1)
            k = 0
            for size in split:
                what = "split %s at tick %d" % (split, k)
                if size == 1:            # a lone gated tick
                    t0, tc, ts = sc.times(k)
                    d = DeviceArray(r.lists[k])
                    d_f, d_e = DeviceArray(np.zeros(len(r.lists[k]), dtype=np.uint8)), DeviceArray(np.zeros(len(r.lists[k])))
                    eng.tick_run_sources_cca_device(t0, t0 + CR.TICK, d.ptr.value, len(r.lists[k]), ts, CR.AIR, tc, sc.threshold, d_f.ptr.value, d_e.ptr.value)
                    eng.sync()
                    _same_sense((DeviceArray.read(d_f.ptr.value, np.uint8, len(r.lists[k])), DeviceArray.read(d_e.ptr.value, np.float64, len(r.lists[k]))),
                                (r.flags[k], r.energy[k]), what)
                    _same_links(eng.result_copy(len(r.lists[k]), cap=1 << 22), r.exp[k], what)
                    for x in (d, d_f, d_e):
                        x.free()
                    assert not _kernels(eng)
                else:
                    got = _batch(eng, sc, r.lists[k:k + size], k, "device", sc.threshold)
                    _check_batch(eng, r, k, k + size, got, what)
                k += size
                _window_is(eng, O, sc, r, k - 1, what)
            assert _kernels(eng) == {"k_ccab_begin", "k_ccab_index<true>", "k_ccab_pairs<true, false>", "k_ccab_scan_sums", "k_ccab_scan_top",
                                     "k_ccab_scan_offsets", "k_ccab_pairs<true, true>", "k_ccab_resolve"}, _kernels(eng)
        finally:
            eng.close()


def test_sixteen_channels(rsa, O):
    sc, r = BR.scene(O, "ch16"), BR.run(O, "ch16", 6)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        _check_batch(eng, r, 0, 6, _batch(eng, sc, r.lists, 0, "device", sc.threshold), "ch16")
        _window_is(eng, O, sc, r, 5, "ch16")
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_the_chain_by_hand(rsa, O, form):
    """A kept in tick 0; B, in A's range, deferred in tick 1; C senses B but not A and is KEPT in tick 2 (an implementation that takes
    every candidate for on the air defers it); A again in tick 3: transmitting; B again in tick 2: deferred, not transmitting."""
    sc, r = BR.scene(O, "chain"), BR.run(O, "chain", 4)
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        got = _batch(eng, sc, r.lists, 0, form, sc.threshold)
        _check_batch(eng, r, 0, 4, got, "chain")
        at = lambda k, node: int(np.flatnonzero(r.lists[k] == node)[0])
        assert got[0][0][at(0, sc.a)] == 0
        assert got[1][0][at(1, sc.b)] == R.ED_BUSY
        assert got[2][0][at(2, sc.c)] == 0
        assert got[3][0][at(3, sc.a)] & R.ED_TRANSMITTING
        assert got[2][0][at(2, sc.b)] == R.ED_BUSY
        _window_is(eng, O, sc, r, 3, "chain")
    finally:
        eng.close()


def test_edge_lists(rsa, O):
    """Short lists (under kEdSmallWindow frames in all: the index without a grid): a tick with n_src = 0 in the middle, a tick that is all
    padding, device-list entries outside 0 .. n_nodes-1; a NaN threshold (only RM_ED_TRANSMITTING defers); a threshold below the noise
    level (everything defers, tick 0 too)."""
    sc = BR.scene(O, "multi")
    base = [s[:40] for s in sc.ticks]
    bad = base[3].copy()
    bad[[2, 9]] = sc.nd.n, -7
    again = np.concatenate([base[0][base[0] >= 0][:12], base[4][:20]])          # nodes of tick 0 once more, two ticks later
    lists = [base[0], np.zeros(0, dtype=np.int32), np.full(10, -1, dtype=np.int32), bad, again, base[5]]
    assert len(np.unique(again[again >= 0])) == (again >= 0).sum()                # (distinct nodes within a tick)
    for thr, what in ((sc.threshold, "edge lists"), (NAN, "NaN threshold"), (-120.0, "below the noise level")):
        r = BR.Run(O, sc, len(lists), threshold=thr, lists=lists)
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            eng.profile_enable(1)
            got = _batch(eng, sc, lists, 0, "device", thr)
            _check_batch(eng, r, 0, len(lists), got, what)
            _window_is(eng, O, sc, r, len(lists) - 1, what)
            assert "k_ccab_index<false>" in _kernels(eng) and "k_ccab_pairs<false, true>" in _kernels(eng), _kernels(eng)
            flags = np.concatenate([g[0] for g in got])
            real = np.concatenate([(s >= 0) & (s < sc.nd.n) for s in lists])
            assert got[3][0][2] == 0 and np.isnan(got[3][1][9]) and not flags[~real].any()
            if thr != thr:
                assert set(flags.tolist()) == {0, R.ED_TRANSMITTING} and (got[4][0][:12] == R.ED_TRANSMITTING).all()
            elif thr == -120.0:
                assert np.all(flags[real] & R.ED_BUSY) and all(eng.batch_result_count(b)[0] == 0 for b in range(len(lists)))
            else:
                assert (flags[real] == 0).any() and (flags[real] != 0).any()
        finally:
            eng.close()


def test_self_contained_batch(rsa, O):
    """Air time <= tick length and an empty window: every energy is the noise level, nothing defers above it, and the results are the
    plain batch's."""
    sc = BR.scene(O, "multi")
    lists = sc.ticks[:5]
    noise = R.channel_energy(O, sc.model(O), sc.nd, np.zeros(0, dtype=O.PACKET_DTYPE), 0, nodes=np.array([0], dtype=np.int32))[0][0]
    a, b = _engine(rsa, sc.nd, sc.params), _engine(rsa, sc.nd, sc.params)
    keep = []
    try:
        got = _batch(a, sc, lists, 0, "device", sc.threshold, air=500)
        tb, te, tc, ts = _times(sc, 0, 5)
        keep = [DeviceArray(s) for s in lists]
        b.batch_run_sources_device(tb, te, [d.ptr.value for d in keep], [len(s) for s in lists], ts, [500] * 5)
        for k, src in enumerate(lists):
            assert not got[k][0].any()
            np.testing.assert_array_equal(_bits(got[k][1][src >= 0]), _bits(np.full(int((src >= 0).sum()), noise)))
            assert np.isnan(got[k][1][src < 0]).all()
            ra, rb = a.batch_result_copy(k, len(src), cap=1 << 22), b.batch_result_copy(k, len(src), cap=1 << 22)
            assert ra.count == rb.count > 0
            for f in ("pkt", "dst", "verdict", "pkt_interference", "pkt_offset"):
                np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg="tick %d: %s" % (k, f))
            for f in ("rssi", "sinr"):
                np.testing.assert_array_equal(_bits(getattr(ra, f)), _bits(getattr(rb, f)), err_msg="tick %d: %s" % (k, f))
    finally:
        for d in keep:
            d.free()
        a.close()
        b.close()


def test_reception_stage_after_a_gated_batch(rsa, O):
    """rm_events_enable, a gated batch, rm_events_process_batch: the deliveries of every tick's drain against O.Sim fed with the KEPT
    frames only, under packet numbers that count the deferred and padding slots."""
    from test_gpu_events_batch import oracle_drain, same_drain
    sc, r = BR.scene(O, "multi"), BR.run(O, "multi", 12)
    eng = _engine(rsa, sc.nd, sc.params)
    sim = O.Sim(sc.nd.n)
    try:
        eng.set_time(0)
        eng.events_enable()
        base = delivered = 0
        got = _batch(eng, sc, r.lists[:6], 0, "device", sc.threshold)
        ends = _times(sc, 0, 6)[1]
        views = eng.events_process_batch(ends)
        for k in range(6):
            _same_sense(got[k], (r.flags[k], r.energy[k]), "tick %d" % k)
            exp = r.exp[k]
            raw = exp.raw
            for q, slot in enumerate(exp.slots):       # one packet at a time, in packet order, under its slot's number
                sel = slice(*np.searchsorted(raw.pkt, [q, q + 1]))
                one = O.TickResult(sel.stop - sel.start, np.zeros(sel.stop - sel.start, dtype=np.int32), raw.dst[sel], raw.verdict[sel],
                                   raw.rssi[sel], raw.sinr[sel], None, None, 0)
                sim.medium_calls(one, exp.new[q:q + 1], pkt_base=base + int(slot))
            base += len(r.lists[k])
            delivered += same_drain(views[k], oracle_drain(O, sim, ends[k]), "tick %d" % k)
        delivered += same_drain(eng.events_process(10 ** 6), oracle_drain(O, sim, 10 ** 6), "final drain")
        assert sim.pending == 0 and delivered > 500 and eng.events_next_packet() == base
        eng.events_disable()
    finally:
        sim.close()
        eng.close()


def _refused(rsa, eng, code, call):
    from radio_sim_amd import _lib
    with pytest.raises(rsa.RadioMediumError) as err:
        call()
    assert err.value.code == code and len(_lib.lib().rm_last_error()) > 0, err.value
    return str(err.value)


def _gated_call(eng, form, tb, te, lists, ts, airs, tc):
    """a gated batch that is expected to be refused: nothing comes back"""
    if form == "host":
        return eng.batch_run_sources_cca(tb, te, lists, ts, airs, tc, -90.0)
    d = [DeviceArray(np.ascontiguousarray(x, dtype=np.int32)) for x in lists]
    try:
        eng.batch_run_sources_cca_device(tb, te, [x.ptr.value for x in d], [len(x) for x in lists], ts, airs, tc, -90.0, None, None)
    finally:
        for x in d:
            x.free()


def test_refusals_of_the_context_state(rsa, O):
    """RM_ERR_STATE: not the SINR medium, a receiver partition, links that can draw in a batch of overlapping ticks, a window selected
    for a region.  Where the context has a window, a query after the refusal finds it as it was."""
    from radio_sim_amd import _lib
    sc = BR.scene(O, "multi")
    nd = sc.nd
    lists = sc.ticks[3:6]
    tb, te, tc, ts = _times(sc, 3, 6)
    airs = [CR.AIR] * 3
    for p in ({"ld_sigma_db": 4.0, "ld_seed": 1}, None):       # not the SINR medium
        eng = rsa.Engine(0)
        try:
            eng.upload_table(nd)
            if p is None:
                eng.set_model(KINDS["udgm"])
            else:
                eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in p.items()})
            for form in ("host", "device"):
                _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, form, tb, te, lists, ts, airs, tc))
        finally:
            eng.close()
    eng = _engine(rsa, nd, sc.params)
    try:
        eng.set_partition(0, nd.n // 2)
        _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, "host", tb, te, lists, ts, airs, tc))
        eng.set_partition_spatial(1, 2)
        _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, "device", tb, te, lists, ts, airs, tc))
    finally:
        eng.close()
    drawing = O.NodeTable(nd.n)                                 # links that can draw, in a batch of overlapping ticks
    drawing.x, drawing.y = nd.x, nd.y
    drawing.rxprob[::3] = 0.6
    eng = _engine(rsa, drawing, sc.params)
    try:
        for form in ("host", "device"):
            _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, form, tb, te, lists, ts, airs, tc))
            energy, flags = eng.channel_energy(tc[0], nodes=lists[0][lists[0] >= 0])
            assert not flags.any() and len(set(_bits(energy).tolist())) == 1          # (nothing on the air: the noise level)
    finally:
        eng.close()
    # a window selected for a region: a gathered batch over a receiver partition leaves frames on the air that were kept for that
    # region only
    eng = _engine(rsa, nd, sc.params)
    d = None
    try:
        eng.set_partition_spatial(0, 2)
        own = eng.partition_of_nodes(2)
        srcs = [s[s >= 0] for s in sc.ticks[:2]]                 # (two overlapping ticks: the batch that keeps frames on the air)
        slots = max(int((own[s] == r).sum()) for s in srcs for r in range(2)) + 1
        packed = np.full((2, 2, slots), -1, dtype=np.int32)
        for b, src in enumerate(srcs):
            for r in range(2):
                mine = src[own[src] == r]
                packed[r, b, :len(mine)] = mine
        d = DeviceArray(packed.reshape(-1))
        eng.batch_run_gathered_sources_device([0, 1000], [1000, 2000], d.ptr.value, 2, slots, [0, 1000], CR.AIR)
        eng.sync()
        for form in ("host", "device"):
            _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, form, tb, te, lists, ts, airs, tc))
        # (the partition cannot be lifted while such frames are on the air, so the refusal of the partition always comes first)
        msg = _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: eng.set_partition(0, nd.n))
        assert "region" in msg, msg
        for form in ("host", "device"):
            _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, form, tb, te, lists, ts, airs, tc))
    finally:
        if d:
            d.free()
        eng.close()


def test_refusals_leave_the_context_as_it_was(rsa, O):
    """Every refusal of the arguments, each followed by a window query and a plain tick that give what the oracle's chain gives without
    the refused call; then a gated batch."""
    from radio_sim_amd import _lib
    from radio_sim_amd.engine import check
    sc = BR.scene(O, "multi")
    nd = sc.nd
    chain = CR.Chain(O, nd, sc.model(O))
    eng = _engine(rsa, nd, sc.params)
    rng = np.random.default_rng(5)
    state = {"k": 0}

    def gated(n_ticks, what):
        k = state["k"]
        lists = [sc.ticks[(k + b) % 12] for b in range(n_ticks)]
        want = [chain.gated_tick(*((sc.times(k + b)[0], lists[b], sc.times(k + b)[2], CR.AIR, sc.times(k + b)[1], sc.threshold))) for b in range(n_ticks)]
        got = _batch(eng, sc, lists, k, "device", sc.threshold)
        for b in range(n_ticks):
            _same_sense(got[b], want[b][:2], "%s, tick %d" % (what, k + b))
            _same_links(eng.batch_result_copy(b, len(lists[b]), cap=1 << 22), want[b][2], "%s, tick %d" % (what, k + b))
        state["k"] = k + n_ticks

    def after(what, t=None):
        """the window through the query, then a plain tick: both as the chain has them"""
        k = state["k"]
        t = sc.times(k - 1)[2] + 1 if t is None else t
        nodes = np.unique(np.concatenate([chain.onair["src"][-200:], rng.integers(0, nd.n, 60)])).astype(np.int32)
        want = R.channel_energy(O, chain.mdl, nd, chain.onair, t, nodes=nodes, threshold=-90.0)
        got = eng.channel_energy(t, nodes=nodes, cca_threshold_dbm=-90.0)
        np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": window flags")
        np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=what + ": window energy")
        t0, _, ts = sc.times(k)
        src = sc.ticks[k % 12][:30]
        dev = DeviceArray(src)
        try:
            eng.tick_run_sources_device(t0, t0 + CR.TICK, dev.ptr.value, len(src), ts, CR.AIR)
            _same_links(eng.result_copy(len(src), cap=1 << 22), chain.plain_tick(t0, src, ts, CR.AIR), what + ": the plain tick that follows")
        finally:
            dev.free()
        state["k"] = k + 1

    def refused(code, form, what, tb=None, tc=None, ts=None, air=None, lists=None):
        """a batch of three ticks at the current clock, with the named arguments replaced (functions of the good values)"""
        k = state["k"]
        b, e, c, s = _times(sc, k, k + 3)
        good = [sc.ticks[(k + i) % 12] for i in range(3)]
        fix = lambda f, v: f(list(v)) if f else v
        _refused(rsa, eng, code, lambda: _gated_call(eng, form, fix(tb, b), e, fix(lists, good), fix(ts, s), fix(air, [CR.AIR] * 3), fix(tc, c)))
        after("%s, %s form" % (what, form))

    def put(i, v):
        def f(lst):
            lst[i] = v(lst) if callable(v) else v
            return lst
        return f

    def bad_entry(v):
        def f(lst):
            lst[1] = lst[1].copy()
            lst[1][3] = v
            return lst
        return f

    try:
        gated(3, "ticks 0 .. 2")
        for form in ("host", "device"):
            refused(_lib.RM_ERR_INVALID, form, "a sample before its tick's t_begin", tc=put(1, lambda c: c[1] - 129))
            refused(_lib.RM_ERR_INVALID, form, "a sample after its tick's start", tc=put(1, lambda c: c[1] + 73))
            refused(_lib.RM_ERR_INVALID, form, "a first sample behind the window's clock", tb=put(0, 1000), tc=put(0, 1200), ts=put(0, 1500))
            refused(_lib.RM_ERR_INVALID, form, "a negative air time", air=put(1, -1))
            refused(_lib.RM_ERR_INVALID, form, "an air time of 2^32 us", air=put(1, 2 ** 32))
            # ticks 0 and 1 swapped in time: tick 1 begins before tick 0, its sample is not behind tick 0's t_begin
            refused(_lib.RM_ERR_STATE, form, "overlapping ticks out of time order", tb=lambda b: [b[1], b[0], b[2]],
                    tc=lambda c: [c[1], c[1], c[2]], ts=lambda s: [s[1], s[1], s[2]])
            refused(_lib.RM_ERR_STATE, form, "an overlapping tick of more than 8192 candidates",
                    lists=put(1, np.arange(8193, dtype=np.int32) % nd.n))
        z = np.zeros(1, dtype=np.int64)
        for n_ticks in (0, -1, 513):                                                    # (RM_MAX_BATCH is 512)
            _refused(rsa, eng, _lib.RM_ERR_INVALID, lambda: check(_lib.lib().rm_batch_run_sources_cca_device(
                eng._h, n_ticks, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, -90.0, None, None)))
            after("n_ticks = %d" % n_ticks)
        for bad in (nd.n, -2, 2 ** 31 - 1):                                             # a host list entry outside -1 .. n-1
            refused(_lib.RM_ERR_INVALID, "host", "host index %d" % bad, lists=bad_entry(bad))
        k = state["k"]
        eng.tick_begin(sc.times(k)[0], sc.times(k)[0] + CR.TICK)
        b, e, c, s = _times(sc, k, k + 3)
        good = [sc.ticks[(k + i) % 12] for i in range(3)]
        for form in ("host", "device"):
            _refused(rsa, eng, _lib.RM_ERR_STATE, lambda: _gated_call(eng, form, b, e, good, s, [CR.AIR] * 3, c))
        eng.enqueue_tx(int(good[0][0]), sc.times(k)[0], CR.AIR)                         # (the host tick goes on: one frame joins the window)
        eng.tick_flush()
        chain.plain_tick(sc.times(k)[0], good[0][:1], sc.times(k)[0], CR.AIR)
        after("between rm_tick_begin and rm_tick_flush", t=sc.times(k)[0] + 1)
        gated(3, "the batch that follows")
    finally:
        eng.close()


def test_the_callers_device_lists_are_unwritten(rsa, O):
    """(_batch compares every device list with what was uploaded, after the call has completed; here with outputs the caller leaves out)"""
    sc, r = BR.scene(O, "multi"), BR.run(O, "multi", 12)
    eng = _engine(rsa, sc.nd, sc.params)
    d = [DeviceArray(s) for s in r.lists[:3]]
    try:
        tb, te, tc, ts = _times(sc, 0, 3)
        eng.batch_run_sources_cca_device(tb, te, [x.ptr.value for x in d], [len(s) for s in r.lists[:3]], ts, [CR.AIR] * 3, tc, sc.threshold)
        eng.sync()
        for x, s in zip(d, r.lists[:3]):
            np.testing.assert_array_equal(DeviceArray.read(x.ptr.value, np.int32, len(s)), s)
        for k in range(3):
            _same_links(eng.batch_result_copy(k, len(r.lists[k]), cap=1 << 22), r.exp[k], "tick %d" % k)
    finally:
        for x in d:
            x.free()
        eng.close()
