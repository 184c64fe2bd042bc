"""The channel energy query (rm_channel_energy*) on the GPU against tests/energy_ref.py, which computes
the expected values from the oracle alone.  Energies are compared bit for bit (float64 viewed as uint64), flags exactly."""
import numpy as np
import pytest

import energy_ref as R
from test_energy_ref import reference_scene
from util import DeviceArray, KINDS, _PARAM_MAP, to_tx_records

pytestmark = pytest.mark.gpu

NOISE = -100.0


def _engine(rsa, nd, params):
    eng = rsa.Engine(0)
    eng.upload_table(nd)
    eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in params.items()})
    return eng


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=what + ": energy bits")
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": flags")


def _device_query(eng, t, n, nodes=None, channel=None, thr=float("nan"), n_out=None):
    """the raw form: device list (or None), device outputs, read back after a synchronise"""
    n_out = n if n_out is None else n_out
    d_nodes = DeviceArray(np.ascontiguousarray(nodes, dtype=np.int32)) if nodes is not None else None
    d_e = DeviceArray(np.full(max(n_out, 1), 12345.0))
    d_f = DeviceArray(np.full(max(n_out, 1), 77, dtype=np.uint8))
    try:
        eng.channel_energy_device(t, d_nodes.ptr.value if d_nodes else None, n, channel, thr, d_e.ptr.value, d_f.ptr.value)
        eng.sync()
        return DeviceArray.read(d_e.ptr.value, np.float64, max(n_out, 1))[:n_out], DeviceArray.read(d_f.ptr.value, np.uint8, max(n_out, 1))[:n_out]
    finally:
        for d in (d_nodes, d_e, d_f):
            if d:
                d.free()


def _tick(eng, nd, srcs, t0, air, tick_us=1000):
    dev = DeviceArray(np.ascontiguousarray(srcs, dtype=np.int32))
    eng.tick_run_sources_device(t0, t0 + tick_us, dev.ptr.value, len(srcs), t0, air)
    eng.sync()
    dev.free()
    return nd.packets(srcs, t0, air)


def test_whole_scene_all_nodes(rsa, O):
    """Reference scene (tests/test_energy_ref.py holds its conditions): every node, host form and device form, at five times."""
    from radio_sim_amd import workload as W
    nd, params, srcs, frames = reference_scene(O)
    mdl = O.model(4, **params)
    eng = _engine(rsa, nd, params)
    try:
        _tick(eng, nd, srcs, 0, W.AIR_US)
        on_air = R.channel_energy(O, mdl, nd, frames, 0, threshold=-90.0)
        assert (on_air[2] >= 4).mean() >= 0.5
        for t in (0, 4000, 8127, 8128, 20_000):
            want = on_air if t < 8128 else R.channel_energy(O, mdl, nd, frames, t, threshold=-90.0)
            if t >= 8128:   # the end of a span is exclusive
                assert np.all(want[0] == NOISE) and not want[1].any()
            _same(eng.channel_energy(t, cca_threshold_dbm=-90.0), want, "host form, t=%d" % t)
            _same(_device_query(eng, t, nd.n, thr=-90.0), want, "device form, t=%d" % t)
    finally:
        eng.close()


@pytest.mark.parametrize("params", [{"ld_sigma_db": 4.0, "ld_seed": 0xC0FFEE, "ld_flags": 1},
                                    {"ld_sigma_db": 0.0, "ld_flags": 1},
                                    {"ld_sigma_db": 4.0, "ld_seed": 7, "ld_clip": 6.0, "ld_flags": 1}],
                         ids=["shadow", "sigma0", "clip6"])
def test_both_kernel_paths(rsa, O, params):
    """100 frames (the small-window path: every live frame swept from LDS) and 400 frames (the grid): the kernels that ran are
    read from rm_profile_kernels, and both paths answer with the reference's bits."""
    from radio_sim_amd import workload as W
    nd, _, _, _ = reference_scene(O)
    mdl = O.model(4, **params)
    sample = np.sort(np.random.default_rng(3).choice(nd.n, 1500, replace=False)).astype(np.int32)
    ran = set()
    for n_frames in (100, 400):
        eng = _engine(rsa, nd, params)
        try:
            eng.profile_enable(1)
            srcs = W.choose_sources(nd.n, n_frames, 0xC0FFEE04, 3)
            frames = _tick(eng, nd, srcs, 0, W.AIR_US)
            want = R.channel_energy(O, mdl, nd, frames, 100, nodes=sample, threshold=-85.0)
            assert (want[2] >= 2).mean() > 0.5
            e, f = eng.channel_energy(100, cca_threshold_dbm=-85.0)
            _same((e[sample], f[sample]), want, "%d frames, all nodes" % n_frames)
            _same(eng.channel_energy(100, nodes=sample, cca_threshold_dbm=-85.0), want, "%d frames, list" % n_frames)
            names = {k for k in eng.profile_kernels() if k.startswith("k_energy")}
            assert names == ({"k_energy_index<false>", "k_energy_sum<false>"} if n_frames == 100 else {"k_energy_index<true>", "k_energy_sum<true>"}), names
            ran |= names
        finally:
            eng.close()
    assert len(ran) == 4


def test_overlapping_frames_across_ticks_four_ways(rsa, O):
    """Eight ticks of 1000 us, 100 new frames of 8128 us each: the window grows to 800 frames.  Fed through the host tick, source
    indices, records in device memory and one batch of overlapping ticks; queried after every tick at t_begin + 500."""
    from radio_sim_amd import workload as W
    nd, params, _, _ = reference_scene(O)
    mdl = O.model(4, **params)
    ticks = [W.choose_sources(nd.n, 100, 0xC0FFEE04, 10 + k) for k in range(8)]
    sample = np.sort(np.random.default_rng(4).choice(nd.n, 600, replace=False)).astype(np.int32)
    sent = np.zeros(0, dtype=O.PACKET_DTYPE)
    want = []
    for k in range(8):
        sent = np.concatenate([sent, nd.packets(ticks[k], 1000 * k, W.AIR_US)])
        want.append(R.channel_energy(O, mdl, nd, sent, 1000 * k + 500, nodes=sample, threshold=-90.0))
    assert (want[-1][2] >= 8).mean() > 0.5
    results = {}
    for way in ("host", "sources", "records", "batch"):
        eng = _engine(rsa, nd, params)
        keep = []
        try:
            got = []
            if way == "batch":
                dev = [DeviceArray(s) for s in ticks]
                keep.extend(dev)
                starts = [1000 * k for k in range(8)]
                eng.batch_run_sources_device(starts, [s + 1000 for s in starts], [d.ptr.value for d in dev], [100] * 8, starts, [W.AIR_US] * 8)
                assert eng.air_batch_stats() == (1, 8)
                got = [None] * 7 + [eng.channel_energy(7500, cca_threshold_dbm=-90.0)]
            for k in range(8 if way != "batch" else 0):
                t0 = 1000 * k
                if way == "host":
                    eng.tick_begin(t0, t0 + 1000)
                    for s in ticks[k]:
                        eng.enqueue_tx(int(s), t0, W.AIR_US)
                    eng.tick_flush(cap=1 << 20)
                elif way == "sources":
                    d = DeviceArray(ticks[k])
                    keep.append(d)
                    eng.tick_run_sources_device(t0, t0 + 1000, d.ptr.value, 100, t0, W.AIR_US)
                else:
                    d = DeviceArray(to_tx_records(rsa, nd.packets(ticks[k], t0, W.AIR_US)))
                    keep.append(d)
                    eng.tick_run_records_device(t0, t0 + 1000, d.ptr.value, 100, t0 + W.AIR_US)
                got.append(eng.channel_energy(t0 + 500, cca_threshold_dbm=-90.0))
            for k in range(8):
                if got[k] is not None:
                    _same((got[k][0][sample], got[k][1][sample]), want[k], "%s, tick %d" % (way, k))
            results[way] = got[7]
        finally:
            for d in keep:
                d.free()
            eng.close()
    for way in ("sources", "records", "batch"):   # every node, not only the sample
        _same(results[way], results["host"], "%s against the host tick" % way)


def test_sixteen_channels(rsa, O):
    from radio_sim_amd import workload as W
    n = 10_000
    src = W.make_nodes(n, 4, channels16=True)
    nd = O.NodeTable(n)
    nd.x, nd.y, nd.channel = src.x, src.y, src.channel
    params = {"ld_sigma_db": 4.0, "ld_seed": 0xC0FFEE, "ld_flags": 1}
    mdl = O.model(4, **params)
    eng = _engine(rsa, nd, params)
    try:
        srcs = W.choose_sources(n, 1600, 0xC0FFEE04, 1)
        frames = _tick(eng, nd, srcs, 0, W.AIR_US)
        sample = np.sort(np.random.default_rng(5).choice(n, 1000, replace=False)).astype(np.int32)
        own = R.channel_energy(O, mdl, nd, frames, 10, nodes=sample, threshold=-92.0)
        ch15 = R.channel_energy(O, mdl, nd, frames, 10, nodes=sample, channel=15, threshold=-92.0)
        assert (own[2] >= 2).mean() > 0.5 and not np.array_equal(own[0], ch15[0])
        e, f = eng.channel_energy(10, cca_threshold_dbm=-92.0)
        _same((e[sample], f[sample]), own, "own channel")
        e, f = eng.channel_energy(10, channel=15, cca_threshold_dbm=-92.0)
        _same((e[sample], f[sample]), ch15, "channel 15 for every node")
        _same(_device_query(eng, 10, len(sample), nodes=sample, channel=15, thr=-92.0), ch15, "channel 15, device list")
    finally:
        eng.close()


def test_moved_nodes(rsa, O):
    """50 nodes move between the tick and the query -- receivers and sources of frames on the air: receivers are where the table
    says now, frames where their records say."""
    from radio_sim_amd import workload as W
    nd, params, srcs, _ = reference_scene(O)
    mdl = O.model(4, **params)
    srcs = W.choose_sources(nd.n, 400, 0xC0FFEE04, 5)
    eng = _engine(rsa, nd, params)
    try:
        frames = _tick(eng, nd, srcs, 0, W.AIR_US)
        before = eng.channel_energy(1)
        rng = np.random.default_rng(6)
        movers = np.concatenate([srcs[:20], rng.choice(np.setdiff1d(np.arange(nd.n), srcs), 30, replace=False)]).astype(np.int32)
        anchors = srcs[rng.integers(20, 400, 50)]
        nd.x[movers], nd.y[movers] = nd.x[anchors] + rng.uniform(2, 30, 50), nd.y[anchors] - rng.uniform(2, 30, 50)
        eng.move_nodes(movers, nd.x[movers], nd.y[movers])
        near = np.unique(np.concatenate([movers, rng.choice(nd.n, 800, replace=False)])).astype(np.int32)
        want = R.channel_energy(O, mdl, nd, frames, 1, nodes=near, threshold=-80.0)
        got = eng.channel_energy(1, cca_threshold_dbm=-80.0)
        _same((got[0][near], got[1][near]), want, "after the move")
        moved_idx = np.searchsorted(near, movers)
        assert not np.array_equal(_bits(before[0][movers]), _bits(want[0][moved_idx]))      # the move matters
        assert np.all(want[1][np.searchsorted(near, srcs[:20])] & R.ED_TRANSMITTING)         # a moved source is still sending
    finally:
        eng.close()


def test_node_lists(rsa, O):
    from radio_sim_amd import workload as W
    nd, params, srcs, frames = reference_scene(O)
    eng = _engine(rsa, nd, params)
    try:
        _tick(eng, nd, srcs, 0, W.AIR_US)
        full = eng.channel_energy(5, cca_threshold_dbm=-90.0)
        rng = np.random.default_rng(7)
        lst = rng.integers(0, nd.n, 3000).astype(np.int32)      # shuffled, with repeats
        lst[:50] = lst[50:100]
        _same(eng.channel_energy(5, nodes=lst, cca_threshold_dbm=-90.0), (full[0][lst], full[1][lst]), "host list")
        _same(_device_query(eng, 5, len(lst), nodes=lst, thr=-90.0), (full[0][lst], full[1][lst]), "device list")
        one = np.array([int(srcs[3])], dtype=np.int32)
        got = eng.channel_energy(5, nodes=one, cca_threshold_dbm=-90.0)
        _same(got, (full[0][one], full[1][one]), "a list of one")
        assert got[1][0] & R.ED_TRANSMITTING
        _same(eng.channel_energy(5, nodes=np.zeros(0, dtype=np.int32)), (np.zeros(0), np.zeros(0, dtype=np.uint8)), "n = 0")
        eng.channel_energy_device(5, None, 0, None, float("nan"), None, None)
        first = _device_query(eng, 5, 37, thr=-90.0)            # no list, fewer than all: nodes 0 .. n-1
        _same(first, (full[0][:37], full[1][:37]), "nodes 0 .. 36")
        bad = np.array([4, -1, 5, nd.n, 6, 2 ** 31 - 1, 7], dtype=np.int32)
        e, f = _device_query(eng, 5, len(bad), nodes=bad, thr=-90.0)
        ok = np.array([0, 2, 4, 6])
        assert np.all(np.isnan(e[[1, 3, 5]])) and not f[[1, 3, 5]].any()
        _same((e[ok], f[ok]), (full[0][bad[ok]], full[1][bad[ok]]), "the neighbours of a bad entry")
        for k in (1, 3):
            with pytest.raises(rsa.RadioMediumError) as err:
                eng.channel_energy(5, nodes=bad[[0, k]])
            assert err.value.code == -1
    finally:
        eng.close()


def test_refusals(rsa, O):
    from radio_sim_amd import _lib
    from radio_sim_amd import workload as W
    nd, params, srcs, _ = reference_scene(O)

    def refused(eng, code, *a, **kw):
        with pytest.raises(rsa.RadioMediumError) as err:
            eng.channel_energy(*a, **kw)
        assert err.value.code == code and len(_lib.lib().rm_last_error()) > 0, err.value

    for p in ({"ld_sigma_db": 4.0, "ld_seed": 1}, None):
        eng = rsa.Engine(0)
        try:
            eng.upload_table(nd)
            if p is None:
                eng.set_model(KINDS["udgm"])
            else:
                eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in p.items()})
            refused(eng, _lib.RM_ERR_STATE, 0)
        finally:
            eng.close()
    eng = _engine(rsa, nd, params)
    try:
        eng.tick_begin(0, 1000)
        refused(eng, _lib.RM_ERR_STATE, 0)
        eng.enqueue_tx(int(srcs[0]), 0, W.AIR_US)
        eng.tick_flush()
        _tick(eng, nd, srcs[1:], 3000, W.AIR_US)
        refused(eng, _lib.RM_ERR_INVALID, 2999)
        eng.channel_energy(3000)
        refused(eng, _lib.RM_ERR_INVALID, 3000, nodes=np.array([nd.n], dtype=np.int32))
    finally:
        eng.close()
    eng = _engine(rsa, nd, params)
    try:
        eng.set_partition(0, nd.n // 2)
        refused(eng, _lib.RM_ERR_STATE, 0)
        eng.set_partition_spatial(1, 2)
        refused(eng, _lib.RM_ERR_STATE, 0)
    finally:
        eng.close()


def test_no_side_effects(rsa, O):
    """Ticks, a batch of overlapping ticks and drains of the reception stage, with queries between every two calls and without:
    heard links, verdicts, sinr, deliveries, the generator, the on-air statistics are identical."""
    from radio_sim_amd import workload as W
    nd, params, _, _ = reference_scene(O)
    nd.rxprob[::5] = 0.6                      # links that draw: the generator's state is part of the comparison
    ticks = [W.choose_sources(nd.n, 100, 0xC0FFEE04, 30 + k) for k in range(9)]

    def run(ask):
        eng = _engine(rsa, nd, params)
        keep, out = [], []
        try:
            eng.seed(99)
            eng.set_time(0)
            eng.events_enable()

            def q(t):
                if ask:
                    eng.channel_energy(t, cca_threshold_dbm=-90.0)
                    _device_query(eng, t, 100, nodes=np.arange(100, dtype=np.int32))

            for k in range(4):
                t0 = 1000 * k
                d = DeviceArray(ticks[k])
                keep.append(d)
                q(t0)
                eng.tick_run_sources_device(t0, t0 + 1000, d.ptr.value, 100, t0, W.AIR_US)
                q(t0 + 1)
                r = eng.result_copy(100)
                out += [r.pkt, r.dst, r.verdict, r.rssi, r.sinr, r.pkt_interference, np.array([eng.rng_state])]
                q(t0 + 2)
                out += [np.asarray(a) for a in eng.events_process(t0 + 1000)[:3]]
            q(4000)
            eng.tick_begin(4000, 5000)
            for s in ticks[4]:
                eng.enqueue_tx(int(s), 4000, W.AIR_US)
            r = eng.tick_flush(cap=1 << 20)
            out += [r.pkt, r.dst, r.verdict, r.rssi, r.sinr, np.array([eng.rng_state])]
            q(4500)
            out += [np.asarray(a) for a in eng.events_process(5000)[:3]]
            eng.events_disable()
            nd1 = O.NodeTable(nd.n)
            nd1.x, nd1.y = nd.x, nd.y
            eng.upload_table(nd1)                  # (a batch of overlapping ticks must not draw)
            q(5000)
            dev = [DeviceArray(s) for s in ticks[5:9]]
            keep.extend(dev)
            starts = [5000 + 1000 * b for b in range(4)]
            eng.batch_run_sources_device(starts, [s + 1000 for s in starts], [d.ptr.value for d in dev], [100] * 4, starts, [W.AIR_US] * 4)
            q(8000)
            for b in range(4):
                r = eng.batch_result_copy(b, 100)
                out += [r.pkt, r.dst, r.verdict, r.rssi, r.sinr]
                q(8000 + b)
            d = DeviceArray(ticks[0])
            keep.append(d)
            eng.tick_run_sources_device(9000, 10000, d.ptr.value, 100, 9000, W.AIR_US)
            r = eng.result_copy(100)
            out += [r.pkt, r.dst, r.verdict, r.rssi, r.sinr]
            out.append(np.array(list(eng.air_list_stats()) + [eng.air_scan_ticks()] + list(eng.air_batch_stats()) + [eng.rng_state]))
            return out
        finally:
            for d in keep:
                d.free()
            eng.close()

    plain, asked = run(False), run(True)
    assert len(plain) == len(asked) > 40 and sum(len(a) for a in plain) > 10_000
    for i, (a, b) in enumerate(zip(plain, asked)):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        np.testing.assert_array_equal(a, b, err_msg="output %d differs when queries are interleaved" % i)


def test_empty_window_and_clock_far_ahead(rsa, O):
    from radio_sim_amd import workload as W
    nd, params, srcs, _ = reference_scene(O)
    eng = _engine(rsa, nd, params)
    try:
        for t in (0, -5, 10 ** 12):
            e, f = eng.channel_energy(t, cca_threshold_dbm=-120.0)
            assert np.all(e == NOISE) and np.all(f == R.ED_BUSY)      # the noise level is above -120 dBm
            e, f = _device_query(eng, t, nd.n)
            assert np.all(e == NOISE) and not f.any()
        _tick(eng, nd, srcs, 0, W.AIR_US)
        assert (eng.channel_energy(8127)[0] > NOISE).mean() > 0.9
        for t in (8128, 10 ** 15, 2 ** 62):
            e, f = eng.channel_energy(t, cca_threshold_dbm=-90.0)
            assert np.all(e == NOISE) and not f.any()
    finally:
        eng.close()


def test_full_size_one_million_nodes(rsa, O):
    """configs[4] shape: 1M nodes, 1000 new frames of 8128 us per 1000 us tick, the window at its steady size (9000 frames).
    All-nodes device query; 500 seeded sample nodes plus the 100 nodes nearest to some source against the reference."""
    from radio_sim_amd import workload as W
    n, per = 1_000_000, 1000
    src = W.make_nodes(n, 5)
    nd = O.NodeTable(n)
    nd.x, nd.y = src.x, src.y
    params = {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 0xC0FFEE}
    mdl = O.model(4, **params)
    eng = _engine(rsa, nd, params)
    try:
        eng.set_link_capacity(1 << 22)
        sent = []
        for k in range(12):
            srcs = W.choose_sources(n, per, 0xC0FFEE05, k)
            sent.append(_tick(eng, nd, srcs, 1000 * k, W.AIR_US))
        t = 11_100
        frames = np.concatenate(sent)
        live = frames[(frames["start_us"] <= t) & (t < frames["start_us"] + frames["air_us"])]
        assert len(live) == 9000
        rng = np.random.default_rng(8)
        pick = live[rng.choice(len(live), 100, replace=False)]
        nearest = []
        for p in pick:     # the node nearest to a source that is not the source itself
            d2 = (nd.x - p["x"]) ** 2 + (nd.y - p["y"]) ** 2
            d2[p["src"]] = np.inf
            nearest.append(int(np.argmin(d2)))
        sample = np.unique(np.concatenate([rng.choice(n, 500, replace=False), nearest])).astype(np.int32)
        want = R.channel_energy(O, mdl, nd, live, t, nodes=sample, threshold=-90.0)
        assert (want[2] >= 4).sum() >= 20
        e, f = _device_query(eng, t, n, thr=-90.0)
        assert np.all(e >= NOISE) and int((f & R.ED_TRANSMITTING != 0).sum()) == len(np.unique(live["src"]))
        _same((e[sample], f[sample]), want, "1M nodes, 9000 frames on the air")
        assert {k for k in _profiled(eng, t)} == {"k_energy_index<true>", "k_energy_sum<true>"}
    finally:
        eng.close()


def _profiled(eng, t):
    eng.profile_enable(1)
    eng.channel_energy(t, nodes=np.arange(10, dtype=np.int32))
    return [k for k in eng.profile_kernels() if k.startswith("k_energy")]
