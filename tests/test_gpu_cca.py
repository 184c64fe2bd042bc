"""The carrier-sense gated tick (rm_tick_run_sources_cca*) on the GPU.  Expected values come from the
oracle alone (tests/cca_ref.py: the sensing from tests/energy_ref.py::channel_energy over the frames on the air when the tick
begins, the tick from the oracle's pass with the kept candidates as its new frames, the deliveries from O.Sim).  Everything is
compared bit for bit: flags, energies, heard sets, order, verdicts, rssi, sinr, pkt_offset, Tx-failure flags."""
import numpy as np
import pytest

import cca_ref as CR
import energy_ref as R
from util import DeviceArray, KINDS, _PARAM_MAP

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _engine(rsa, nd, params, cap=None):
    eng = rsa.Engine(0)
    eng.upload_table(nd)
    eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in params.items()})
    if cap:
        eng.set_link_capacity(cap)
    return eng


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_sense(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": flags")
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]), err_msg=what + ": energy bits")


def _same_links(gpu, exp, what):
    assert gpu.count == exp.count, (what, gpu.count, exp.count)
    np.testing.assert_array_equal(gpu.pkt, exp.pkt, err_msg=what + ": pkt")
    np.testing.assert_array_equal(gpu.dst, exp.dst, err_msg=what + ": dst")
    np.testing.assert_array_equal(gpu.verdict, exp.verdict, err_msg=what + ": verdict")
    np.testing.assert_array_equal(_bits(gpu.rssi), _bits(exp.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(gpu.sinr), _bits(exp.sinr), err_msg=what + ": sinr")
    np.testing.assert_array_equal(gpu.pkt_offset, exp.pkt_offset, err_msg=what + ": pkt_offset")
    np.testing.assert_array_equal(gpu.pkt_interference[exp.slots], exp.pkt_interference, err_msg=what + ": Tx-failure flags")


def _gated(eng, form, t0, src, ts, air, tc, thr):
    """one gated tick -> (flags, energy); the device form through device arrays, with the caller's list checked to be unwritten"""
    src = np.ascontiguousarray(src, dtype=np.int32)
    n = len(src)
    if form == "host":
        return eng.tick_run_sources_cca(t0, t0 + CR.TICK, src, ts, air, tc, thr)
    d_s = DeviceArray(src) if n else None
    d_f = DeviceArray(np.full(max(n, 1), 77, dtype=np.uint8))
    d_e = DeviceArray(np.full(max(n, 1), 12345.0))
    try:
        eng.tick_run_sources_cca_device(t0, t0 + CR.TICK, d_s.ptr.value if d_s else None, n, ts, air, tc, thr, d_f.ptr.value, d_e.ptr.value)
        eng.sync()
        if n:
            np.testing.assert_array_equal(DeviceArray.read(d_s.ptr.value, np.int32, n), src, err_msg="the caller's dev_src was written")
        return DeviceArray.read(d_f.ptr.value, np.uint8, max(n, 1))[:n], DeviceArray.read(d_e.ptr.value, np.float64, max(n, 1))[:n]
    finally:
        for d in (d_s, d_f, d_e):
            if d:
                d.free()


def _window_is(eng, O, chain, t, nodes, what):
    """the frames on the air after a tick, through the query: a deferred frame must not be there, a kept one must"""
    nodes = np.unique(nodes[(nodes >= 0) & (nodes < chain.nd.n)]).astype(np.int32)
    want = R.channel_energy(O, chain.mdl, chain.nd, chain.onair, t, nodes=nodes, threshold=-90.0)
    got = eng.channel_energy(t, nodes=nodes, cca_threshold_dbm=-90.0)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": window flags")
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=what + ": window energy")


def _run_scene(rsa, O, sc, form, ticks=None, profile=False):
    chain = CR.Chain(O, sc.nd, sc.model(O))
    eng = _engine(rsa, sc.nd, sc.params)
    seen = []
    try:
        if profile:
            eng.profile_enable(1)
        rng = np.random.default_rng(77)
        deferred = kept = 0
        for k, src in enumerate(sc.ticks[:ticks]):
            t0, tc, ts = sc.times(k)
            what = "%s, %s form, tick %d" % (sc.name, form, k)
            want_f, want_e, exp = chain.gated_tick(t0, src, ts, CR.AIR, tc, sc.threshold)
            got = _gated(eng, form, t0, src, ts, CR.AIR, tc, sc.threshold)
            _same_sense(got, (want_f, want_e), what)
            _same_links(eng.result_copy(len(src), cap=1 << 22), exp, what)
            if profile:
                seen.append({name for name in eng.profile_kernels() if name.startswith(("k_cca", "k_energy"))})
            else:
                _window_is(eng, O, chain, ts + 1, np.concatenate([src, rng.integers(0, sc.nd.n, 100).astype(np.int32)]), what)
            deferred += int((want_f != 0).sum())
            kept += len(exp.slots)
        assert deferred > 0 and kept > 0
        return seen
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_multi_tick_scene(rsa, O, form):
    """Twelve gated ticks over 6000 nodes with shadowing, frames of 8128 us over 1000 us ticks (tests/test_cca_ref.py holds the
    scene's conditions): flags, energies and the tick against the oracle's chain, and the window after every tick through
    rm_channel_energy -- the candidates themselves among the queried nodes: a kept one is transmitting, a deferred one is not."""
    _run_scene(rsa, O, CR.Scene(O, "multi"), form)


def test_sixteen_channels(rsa, O):
    _run_scene(rsa, O, CR.Scene(O, "ch16"), "device", ticks=6)


def test_both_kernel_paths(rsa, O):
    """The window holds 0, 150, 300, 450 records when ticks 0 .. 3 of the scene begin: below kEdSmallWindow (256) the gate has no
    grid.  The kernels that ran are read from rm_profile_kernels; a plain query still runs k_energy_sum."""
    sc = CR.Scene(O, "multi")
    seen = _run_scene(rsa, O, sc, "device", ticks=4, profile=True)
    assert seen[0] == {"k_cca_gate<false>"}, seen[0]                     # (an empty window: nothing to index)
    assert seen[1] == {"k_cca_gate<false>", "k_energy_index<false>"}, seen[1]
    assert seen[3] == {"k_cca_gate<false>", "k_energy_index<false>", "k_cca_gate<true>", "k_energy_index<true>"}, seen[3]
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        d = DeviceArray(sc.ticks[0])
        eng.tick_run_sources_device(0, 1000, d.ptr.value, len(sc.ticks[0]), 0, CR.AIR)
        eng.profile_enable(1)
        eng.channel_energy(10, nodes=sc.ticks[1][sc.ticks[1] >= 0])
        assert {k for k in eng.profile_kernels() if k.startswith(("k_cca", "k_energy"))} == {"k_energy_index<false>", "k_energy_sum<false>"}
        d.free()
    finally:
        eng.close()


def test_equivalence_with_query_filter_and_plain_tick(rsa, O):
    """Inside the engine: a second context does what the gated tick replaces -- rm_channel_energy for the candidates, the busy ones
    struck from the list on the host, rm_tick_run_sources_device with -1 entries.  Flags, energies, every result array (the
    padding slots' Tx-failure flags included), the generator and the ticks that follow are identical.  Some receivers draw."""
    sc = CR.Scene(O, "multi")
    nd = sc.nd
    nd.rxprob[::4] = 0.7
    a, b = _engine(rsa, nd, sc.params), _engine(rsa, nd, sc.params)
    keep = []
    try:
        a.seed(5)
        b.seed(5)
        deferred = 0
        for k, src in enumerate(sc.ticks[:8]):
            t0, tc, ts = sc.times(k)
            if k == 6:          # a plain tick in between, the same in both
                for eng in (a, b):
                    d = DeviceArray(src)
                    keep.append(d)
                    eng.tick_run_sources_device(t0, t0 + CR.TICK, d.ptr.value, len(src), ts, CR.AIR)
            else:
                fa, ea = _gated(a, "device" if k % 2 else "host", t0, src, ts, CR.AIR, tc, sc.threshold)
                real = np.flatnonzero(src >= 0)
                fb, eb = np.zeros(len(src), dtype=np.uint8), np.full(len(src), np.nan)
                eb[real], fb[real] = b.channel_energy(tc, nodes=src[real], cca_threshold_dbm=sc.threshold)
                _same_sense((fa, ea), (fb, eb), "tick %d" % k)
                d = DeviceArray(np.where(fb != 0, -1, src).astype(np.int32))
                keep.append(d)
                b.tick_run_sources_device(t0, t0 + CR.TICK, d.ptr.value, len(src), ts, CR.AIR)
                deferred += int((fb != 0).sum())
            ra, rb = a.result_copy(len(src), cap=1 << 22), b.result_copy(len(src), cap=1 << 22)
            assert ra.count == rb.count > 0
            for f in ("pkt", "dst", "verdict", "pkt_interference", "pkt_offset"):
                np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg="tick %d: %s" % (k, f))
            for f in ("rssi", "sinr"):
                np.testing.assert_array_equal(_bits(getattr(ra, f)), _bits(getattr(rb, f)), err_msg="tick %d: %s" % (k, f))
            assert a.rng_state == b.rng_state
        assert deferred > 100
        assert a.air_list_stats() == b.air_list_stats() and a.air_scan_ticks() == b.air_scan_ticks()
        ea, eb = a.channel_energy(8000), b.channel_energy(8000)
        np.testing.assert_array_equal(ea[1], eb[1])
        np.testing.assert_array_equal(_bits(ea[0]), _bits(eb[0]))
    finally:
        for d in keep:
            d.free()
        a.close()
        b.close()


def test_receivers_that_draw_leave_the_oracles_generator(rsa, O):
    """rxprob < 1 on a third of the nodes: the links of the kept packets draw from java.util.Random in the reference's order, a
    deferred packet draws nothing -- the verdicts and the generator's state after every tick are the oracle's."""
    sc = CR.Scene(O, "multi")
    sc.nd.rxprob[::3] = 0.6
    chain = CR.Chain(O, sc.nd, sc.model(O))
    eng = _engine(rsa, sc.nd, sc.params)
    try:
        eng.seed(1234)
        state = O.lib().orc_jrandom_seed(1234)
        draws = 0
        for k, src in enumerate(sc.ticks[:8]):
            t0, tc, ts = sc.times(k)
            want_f, want_e, exp = chain.gated_tick(t0, src, ts, CR.AIR, tc, sc.threshold, rng_state=state)
            _same_sense(_gated(eng, "device", t0, src, ts, CR.AIR, tc, sc.threshold), (want_f, want_e), "tick %d" % k)
            _same_links(eng.result_copy(len(src), cap=1 << 22), exp, "tick %d" % k)
            assert exp.rng_state != state and eng.rng_state == exp.rng_state, "tick %d: generator" % k
            draws += int(exp.raw.pkt_draws.sum())
            state = exp.rng_state
        assert draws > 1000
    finally:
        eng.close()


def test_moved_nodes_a_far_node_thresholds_and_empty_lists(rsa, O):
    """Nodes move between ticks (a candidate is sensed where the table says now, a frame counts from where its record says); a
    candidate far outside the fp32 frame; a NaN threshold (only a transmitting candidate defers); n = 0; a threshold below the
    noise level (every candidate defers: an all-padding tick) and one nothing reaches."""
    sc = CR.Scene(O, "multi")
    nd = sc.nd
    chain = CR.Chain(O, nd, sc.model(O))
    eng = _engine(rsa, nd, sc.params)
    rng = np.random.default_rng(11)
    try:
        def tick(k, src, thr, what, form="device"):
            t0, tc, ts = sc.times(k)
            want_f, want_e, exp = chain.gated_tick(t0, src, ts, CR.AIR, tc, thr)
            _same_sense(_gated(eng, form, t0, src, ts, CR.AIR, tc, thr), (want_f, want_e), what)
            _same_links(eng.result_copy(len(src), cap=1 << 22), exp, what)
            _window_is(eng, O, chain, ts + 1, np.concatenate([src, rng.integers(0, nd.n, 60).astype(np.int32)]), what)
            return want_f, exp

        tick(0, sc.ticks[0], sc.threshold, "tick 0")
        f1, e1 = tick(1, sc.ticks[1], sc.threshold, "tick 1")
        # sources of frames on the air and candidates of the next tick move next to other frames' sources
        on = chain.onair["src"]
        movers = np.unique(np.concatenate([on[:15], sc.ticks[2][:25]])).astype(np.int32)
        anchors = on[rng.integers(15, len(on), len(movers))]
        nd.x[movers], nd.y[movers] = nd.x[anchors] + rng.uniform(2, 25, len(movers)), nd.y[anchors] - rng.uniform(2, 25, len(movers))
        eng.move_nodes(movers, nd.x[movers], nd.y[movers])
        f2, _ = tick(2, sc.ticks[2], sc.threshold, "after the move")
        assert (f2[:25] & R.ED_BUSY).sum() >= 5
        # a candidate far outside the frame (and a receiver of nothing there)
        far = int(sc.ticks[3][7])
        nd.x[far], nd.y[far] = nd.x[far] + 3.0e6, nd.y[far] - 2.0e6
        eng.move_nodes(np.array([far], dtype=np.int32), nd.x[[far]], nd.y[[far]])
        f3, _ = tick(3, sc.ticks[3], sc.threshold, "a far candidate")
        assert not (f3[7] & R.ED_BUSY)                   # (nothing reaches it)
        # NaN: BUSY is never set; candidates that are on the air themselves still defer
        src4 = np.concatenate([sc.ticks[4], chain.onair["src"][-20:]]).astype(np.int32)
        f4, _ = tick(4, src4, NAN, "NaN threshold", form="host")
        assert not (f4 & R.ED_BUSY).any() and np.all(f4[-20:] == R.ED_TRANSMITTING)
        f5, e5 = tick(5, np.zeros(0, dtype=np.int32), sc.threshold, "n = 0")
        f5, e5 = tick(5, np.zeros(0, dtype=np.int32), sc.threshold, "n = 0, host form", form="host")
        f6, e6 = tick(6, sc.ticks[6], -120.0, "everything deferred")
        assert np.all(f6 & R.ED_BUSY) and e6.count == 0 and not e6.pkt_offset.any()
        f7, e7 = tick(7, sc.ticks[7], 100.0, "nothing busy")
        assert not (f7 & R.ED_BUSY).any() and len(e7.slots) > 100
        tick(8, sc.ticks[8], sc.threshold, "and on")
    finally:
        eng.close()


def test_reception_stage_counts_deferred_slots(rsa, O):
    """With rm_events_enable: the deliveries of every drain and rm_node_info against O.Sim fed with the KEPT packets only, under
    packet numbers that count the deferred and padding slots."""
    from test_gpu_events import check_drain
    sc = CR.Scene(O, "multi")
    chain = CR.Chain(O, sc.nd, sc.model(O))
    eng = _engine(rsa, sc.nd, sc.params)
    sim = O.Sim(sc.nd.n)
    try:
        eng.set_time(0)
        eng.events_enable()
        eng._reported = None
        base = delivered = 0
        for k, src in enumerate(sc.ticks[:6]):
            t0, tc, ts = sc.times(k)
            assert eng.events_next_packet() == base
            want_f, want_e, exp = chain.gated_tick(t0, src, ts, CR.AIR, tc, sc.threshold)
            _same_sense(_gated(eng, "device", t0, src, ts, CR.AIR, tc, sc.threshold), (want_f, want_e), "tick %d" % k)
            raw = exp.raw
            for q, slot in enumerate(exp.slots):       # one packet at a time, in packet order, under its slot's number
                sel = slice(*np.searchsorted(raw.pkt, [q, q + 1]))
                one = O.TickResult(sel.stop - sel.start, np.zeros(sel.stop - sel.start, dtype=np.int32), raw.dst[sel], raw.verdict[sel],
                                   raw.rssi[sel], raw.sinr[sel], None, None, 0)
                sim.medium_calls(one, exp.new[q:q + 1], pkt_base=base + int(slot))
            base += len(src)
            delivered += check_drain(O, eng, sim, t0 + CR.TICK, sc.nd, "tick %d" % k)
        delivered += check_drain(O, eng, sim, 10 ** 6, sc.nd, "final drain")
        assert sim.pending == 0 and delivered > 500 and eng.events_next_packet() == base
        eng.events_disable()
    finally:
        sim.close()
        eng.close()


def test_refusals_leave_the_context_as_it_was(rsa, O):
    from radio_sim_amd import _lib
    sc = CR.Scene(O, "multi")
    nd, src = sc.nd, sc.ticks[0]

    def refused(eng, code, t0, src, ts, tc, form="host", air=CR.AIR):
        with pytest.raises(rsa.RadioMediumError) as err:
            _gated(eng, form, t0, src, ts, air, tc, -90.0)
        assert err.value.code == code and len(_lib.lib().rm_last_error()) > 0, err.value

    for p in ({"ld_sigma_db": 4.0, "ld_seed": 1}, None):       # not the SINR medium
        eng = rsa.Engine(0)
        try:
            eng.upload_table(nd)
            if p is None:
                eng.set_model(KINDS["udgm"])
            else:
                eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in p.items()})
            for form in ("host", "device"):
                refused(eng, _lib.RM_ERR_STATE, 0, src, 0, 0, form)
        finally:
            eng.close()
    eng = _engine(rsa, nd, sc.params)
    try:
        eng.set_partition(0, nd.n // 2)
        refused(eng, _lib.RM_ERR_STATE, 0, src, 0, 0)
        eng.set_partition_spatial(1, 2)
        refused(eng, _lib.RM_ERR_STATE, 0, src, 0, 0, "device")
    finally:
        eng.close()
    chain = CR.Chain(O, nd, sc.model(O))
    eng = _engine(rsa, nd, sc.params)
    try:
        def good(k):
            t0, tc, ts = sc.times(k)
            want_f, want_e, exp = chain.gated_tick(t0, sc.ticks[k], ts, CR.AIR, tc, sc.threshold)
            _same_sense(_gated(eng, "device", t0, sc.ticks[k], ts, CR.AIR, tc, sc.threshold), (want_f, want_e), "tick %d" % k)
            _same_links(eng.result_copy(len(sc.ticks[k]), cap=1 << 22), exp, "tick %d" % k)

        for k in range(3):
            good(k)
        for form in ("host", "device"):
            refused(eng, _lib.RM_ERR_INVALID, 3000, src, 3200, 2999, form)        # a sample before t_begin
            refused(eng, _lib.RM_ERR_INVALID, 3000, src, 3200, 3201, form)        # ... after the start
            refused(eng, _lib.RM_ERR_INVALID, 1000, src, 1500, 1200, form)        # ... behind the latest t_begin of the window
            refused(eng, _lib.RM_ERR_INVALID, 3000, src, 3200, 3100, form, air=-1)
            refused(eng, _lib.RM_ERR_INVALID, 3000, src, 3200, 3100, form, air=2 ** 32)
        for bad in (nd.n, -2, 2 ** 31 - 1):                                       # a host list entry outside -1 .. n-1
            lst = src.copy()
            lst[3] = bad
            refused(eng, _lib.RM_ERR_INVALID, 3000, lst, 3200, 3100)
        eng.tick_begin(3000, 4000)
        refused(eng, _lib.RM_ERR_STATE, 3000, src, 3200, 3100)
        refused(eng, _lib.RM_ERR_STATE, 3000, src, 3200, 3100, "device")
        eng.enqueue_tx(int(src[0]), 3000, CR.AIR)                                 # (the host tick goes on: one frame joins the window)
        eng.tick_flush()
        chain.plain_tick(3000, src[:1], 3000, CR.AIR)
        # in a device list an entry out of range is padding
        lst = sc.ticks[3].copy()
        lst[[2, 9]] = nd.n, -7
        t0, tc, ts = sc.times(3)
        want_f, want_e, exp = chain.gated_tick(t0, lst, ts, CR.AIR, tc, sc.threshold)
        assert want_f[2] == 0 and np.isnan(want_e[9])
        _same_sense(_gated(eng, "device", t0, lst, ts, CR.AIR, tc, sc.threshold), (want_f, want_e), "bad entries in a device list")
        _same_links(eng.result_copy(len(lst), cap=1 << 22), exp, "bad entries in a device list")
        good(4)
        good(5)
    finally:
        eng.close()


def test_full_size_one_million_nodes(rsa, O):
    """configs[4] shape: 1 M nodes, 1000 new frames of 8128 us per 1000 us tick, the window at its steady size (9000 frames live),
    then one gated tick of 1000 candidates: seeded nodes, the nodes nearest to some source on the air, and sources themselves.
    Flags and energies of all candidates against the reference walk (1000 x 9000 pairs), the tick against orc_tick_mt."""
    from radio_sim_amd import workload as W
    n, per = 1_000_000, 1000
    src = W.make_nodes(n, 5)
    nd = O.NodeTable(n)
    nd.x, nd.y = src.x, src.y
    params = {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 0xC0FFEE}
    chain = CR.Chain(O, nd, O.model(O.MODEL_LOGDIST, **params))
    eng = _engine(rsa, nd, params, cap=1 << 22)
    try:
        for k in range(12):
            srcs = W.choose_sources(n, per, 0xC0FFEE05, k)
            d = DeviceArray(srcs)
            eng.tick_run_sources_device(1000 * k, 1000 * k + 1000, d.ptr.value, per, 1000 * k, W.AIR_US)
            eng.sync()
            d.free()
            chain.onair = np.concatenate([chain.onair, nd.packets(srcs, 1000 * k, W.AIR_US)])
        t0, tc, ts = 12_000, 12_050, 12_100
        chain.expire(t0)
        live = chain.onair[(chain.onair["start_us"] <= tc) & (tc < chain.onair["start_us"] + chain.onair["air_us"])]
        assert len(live) == 8000 and len(chain.onair) == 8000      # (the frames of ticks 4 .. 11; tick 12's own would make 9000)
        rng = np.random.default_rng(12)
        nearest = []
        for p in live[rng.choice(len(live), 400, replace=False)]:
            d2 = (nd.x - p["x"]) ** 2 + (nd.y - p["y"]) ** 2
            d2[p["src"]] = np.inf
            nearest.append(int(np.argmin(d2)))
        cand = np.concatenate([rng.choice(n, 550, replace=False), nearest, live["src"][rng.choice(len(live), 50, replace=False)]]).astype(np.int32)
        rng.shuffle(cand)
        assert len(cand) == 1000
        eng.profile_enable(1)
        want_f, want_e, exp = chain.gated_tick(t0, cand, ts, W.AIR_US, tc, -90.0)
        share = (want_f != 0).mean()
        assert 0.10 <= share <= 0.90 and (want_f == R.ED_TRANSMITTING).any() and (want_f == R.ED_BUSY).any(), share
        _same_sense(_gated(eng, "device", t0, cand, ts, W.AIR_US, tc, -90.0), (want_f, want_e), "1M nodes")
        _same_links(eng.result_copy(len(cand), cap=1 << 22), exp, "1M nodes")
        assert {k for k in eng.profile_kernels() if k.startswith(("k_cca", "k_energy"))} == {"k_energy_index<true>", "k_cca_gate<true>"}
    finally:
        eng.close()
