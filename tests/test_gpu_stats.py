"""Per-node traffic counters accumulated on the device (rm_stats_*, rm_stats.hip) on the GPU.  Expected
tables come from the oracle through tests/stats_ref.py alone (tests/test_stats_ref.py holds the scenes' conditions for that
reference).  Every comparison is exact integer equality of whole tables."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cca_batch_ref as BR
import csma_carry_ref as KR
import csma_ref as SR
import errmodel_ref as R
import stats_ref as S
from test_gpu_cca import _bits, _engine as _plain_engine
from test_gpu_cca_batch import _refused
from test_gpu_csma_carry import _part
from util import DeviceArray, assert_same, configure_engine, to_tx_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK = R.TICK
STATS_KERNELS = ("k_stats", "k_stats_batch", "k_rows_gather", "k_rows_scatter")
INVALID, STATE = -1, -5


def _engine(rsa, nd, params=R.PARAMS, stats=True, em_seed=None, cap=None):
    eng = _plain_engine(rsa, nd, params, cap)
    if em_seed is not None:
        eng.set_error_model(rsa.EM_OQPSK_250K, seed=em_seed)
    if stats:
        eng.stats_enable()
    return eng


def _same_links(a, b, what):
    """two engine results, bit for bit"""
    assert a.count == b.count, (what, a.count, b.count)
    for f in ("dst", "verdict", "pkt_offset", "pkt_interference"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg="%s: %s" % (what, f))
    if a.pkt is not None and b.pkt is not None:
        np.testing.assert_array_equal(a.pkt, b.pkt, err_msg=what + ": pkt")
    np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr), err_msg=what + ": sinr")


def _packets(nd, srcs, start, air):
    srcs = np.asarray(srcs, dtype=np.int32)
    new = nd.packets(np.where(srcs >= 0, srcs, 0), start, air)
    new["src"] = srcs
    return new


def _replay_table(nd, lists, starts, air, em_seed=None):
    """the reference table of a run of ticks on the SINR medium (em_seed: with E10's verdicts) -> Table, [TickResult]"""
    rep = R.Replay(nd, seed=R.SEED if em_seed is None else em_seed)
    t, res = S.Table(nd.n), []
    for l, s in zip(lists, starts):
        w, _ = rep.tick(s, l, s, air)
        res.append(w)
        t.add_result(_packets(nd, l, s, air), w, verdict=w.plain if em_seed is None else None)
    return t, res


_REF = {}


def _batch_ref(overlap, em_seed=None):
    """computed once per scene, shared and left unchanged"""
    key = (overlap, em_seed)
    if key not in _REF:
        nd, lists, starts, air = R.scene_batch(overlap)
        _REF[key] = (nd, lists, starts, air) + _replay_table(nd, lists, starts, air, em_seed)
    return _REF[key]


def _run_batch(eng, lists, starts, air, dev):
    arrs = [DeviceArray(s) if len(s) else None for s in lists]
    dev.extend(a for a in arrs if a is not None)
    eng.batch_run_sources_device(starts, [s + TICK for s in starts], [a.ptr.value if a is not None else 0 for a in arrs],
                                 [len(s) for s in lists], starts, [air] * len(lists))


def _lone(eng, form, d, srcs, start, air, t0=0):
    if form == "sources":
        eng.tick_run_sources_device(t0, t0 + TICK, d.ptr.value if d is not None else 0, len(srcs), start, air)
        return eng.result_copy(len(srcs), cap=1 << 20) if len(srcs) else None   # (an empty tick has nothing to read)
    eng.tick_begin(t0, t0 + TICK)
    for s in srcs:
        eng.enqueue_tx(int(s), start, air)
    return eng.tick_flush(cap=1 << 20) if form == "flush" else eng.tick_flush_view()


# ---- 1. every lone form on the SINR medium --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["flush", "view", "sources"])
def test_lone_forms(rsa, O, form):
    nd, srcs, start, air = R.scene_lone()
    want, res = _replay_table(nd, [srcs], [start], air)
    on, off, d = _engine(rsa, nd), _engine(rsa, nd, stats=False), DeviceArray(srcs)
    try:
        assert on.stats_enabled() and not off.stats_enabled()
        got, plain = _lone(on, form, d, srcs, start, air), _lone(off, form, d, srcs, start, air)
        _same_links(got, plain, form + ": statistics on against off")
        np.testing.assert_array_equal(got.dst, res[0].dst)
        np.testing.assert_array_equal(got.verdict, res[0].plain)
        tbl, tot = on.stats_read()
        S.equal(tbl, want, form)
        assert tot == {"ticks_counted": 1, "ticks_skipped": 0}
    finally:
        d.free()
        on.close()
        off.close()


def test_transmit_packet_by_packet(rsa, O):
    nd, srcs, starts, hex_len, air = R.scene_serial()
    want, res = _replay_table(nd, [[q] for q in srcs], [int(s) for s in starts], air)
    on, off = _engine(rsa, nd), _engine(rsa, nd, stats=False)
    try:
        for k, (q, s) in enumerate(zip(srcs, starts)):
            a, b = on.transmit(int(q), int(s), hex_len, cap=1 << 16), off.transmit(int(q), int(s), hex_len, cap=1 << 16)
            assert a.count == b.count == res[k].count
            np.testing.assert_array_equal(a.dst, b.dst)
            np.testing.assert_array_equal(a.verdict, b.verdict)
            np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr))
            np.testing.assert_array_equal(a.dst, res[k].dst)
        tbl, tot = on.stats_read()
        S.equal(tbl, want, "rm_transmit")
        assert tot["ticks_counted"] == len(srcs)
    finally:
        on.close()
        off.close()


# ---- 2. batches of both SINR kinds ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [False, True])
def test_batches_of_both_kinds(rsa, O, overlap):
    nd, lists, starts, air, want, res = _batch_ref(overlap)
    a, b, dev = _engine(rsa, nd), _engine(rsa, nd), []
    try:
        _run_batch(a, lists, starts, air, dev)
        assert a.air_batch_stats()[0] == (1 if overlap else 0)
        tbl, tot = a.stats_read()
        S.equal(tbl, want, "batch")
        assert tot == {"ticks_counted": sum(1 for l in lists if len(l)), "ticks_skipped": 0}
        for k, w in enumerate(res):   # the links are still the oracle's
            got = a.batch_result_copy(k, len(lists[k]), cap=1 << 20)
            assert got.count == w.count
            np.testing.assert_array_equal(got.dst, w.dst)
            np.testing.assert_array_equal(got.verdict, w.plain)
        # the same ticks as lone ticks on a second context
        for l, s in zip(lists, starts):
            d = DeviceArray(l) if len(l) else None
            if d is not None:
                dev.append(d)
            _lone(b, "sources", d, l, s, air, t0=s)
        tbl2, tot2 = b.stats_read()
        S.equal(tbl2, want, "lone ticks")
        np.testing.assert_array_equal(tbl, tbl2)
        assert tot2 == tot
    finally:
        for d in dev:
            d.free()
        a.close()
        b.close()


# ---- 3. the other media ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["udgm", "udgm_const", "n2n"])
def test_reference_media(rsa, O, name):
    scene = {"udgm": S.scene_udgm, "udgm_const": S.scene_udgm_const, "n2n": S.scene_n2n}[name]()
    nd, kind, params, pk, matrix, seed = scene
    cpu = S.oracle_tick(scene)
    want = S.table_of(scene, cpu)
    eng = rsa.Engine(0)
    try:
        configure_engine(eng, nd, kind, params, matrix)
        if seed is not None:
            eng.seed(seed)
        eng.stats_enable()
        gpu = eng.tick(to_tx_records(rsa, pk), cap=1 << 20)
        assert_same(gpu, cpu, name)
        if seed is not None:   # the draw kernels ran, and the pass left the generator alone
            assert cpu.pkt_draws.sum() > 0 and eng.rng_state == cpu.rng_state
        tbl, tot = eng.stats_read()
        S.equal(tbl, want, name)
        assert tot == {"ticks_counted": 1, "ticks_skipped": 0}
    finally:
        eng.close()


def test_null_medium_through_the_dense_tick(rsa, O):
    scene = S.scene_null()
    nd, kind, params, pk, _, _ = scene
    cpu = S.oracle_tick(scene)
    want = S.table_of(scene, cpu)
    srcs = np.ascontiguousarray(pk["src"], dtype=np.int32)
    eng, d = rsa.Engine(0), DeviceArray(srcs)
    try:
        configure_engine(eng, nd, kind, params)
        eng.set_link_capacity(1 << 20)
        eng.stats_enable()
        eng.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, S.AIR)
        if os.environ.get("RM_DENSE_TICK") != "0":   # (a run whose knobs never take the dense form has no masks to ask for)
            r = eng.result_dense()   # the masks still answer before anybody reads records
            assert r.n_packets == len(srcs)
            counts = DeviceArray.read(r.cell_count, np.uint32, len(srcs) * r.chunks).reshape(len(srcs), r.chunks)
            np.testing.assert_array_equal(counts.sum(axis=1), np.bincount(cpu.pkt, minlength=len(srcs)))
        tbl, tot = eng.stats_read()
        S.equal(tbl, want, "null, dense")
        assert tot["ticks_counted"] == 1
        assert_same(eng.result_copy(len(srcs), cap=1 << 20), cpu, "null records")
    finally:
        d.free()
        eng.close()


def test_transmit_on_udgm_returns_the_same_links(rsa, O):
    """a reference medium's rm_transmit leaves its one-launch shortcut while counting: the links are the same, the table is right"""
    nd, _, _, pk, _, _ = S.scene_udgm_const()
    air = int(O.lib().orc_air_time_us(254))
    on, off = rsa.Engine(0), rsa.Engine(0)
    try:
        want = S.Table(nd.n)
        for eng in (on, off):
            configure_engine(eng, nd, "udgm", {})
        on.stats_enable()
        for src in pk["src"][:12]:
            q = nd.packets([int(src)], 0, air)
            cpu = S.oracle_tick((nd, "udgm", {}, q, None, None))
            want.add_result(q, cpu)
            a, b = on.transmit(int(src), 0, 254, cap=1 << 12), off.transmit(int(src), 0, 254, cap=1 << 12)
            assert a.count == b.count == cpu.count > 0
            np.testing.assert_array_equal(a.dst, b.dst)
            np.testing.assert_array_equal(a.verdict, b.verdict)
            np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi))
            np.testing.assert_array_equal(a.dst, cpu.dst)
            np.testing.assert_array_equal(a.verdict, cpu.verdict)
        S.equal(on.stats_read()[0], want, "rm_transmit on UDGM")
    finally:
        on.close()
        off.close()


# ---- 4. with the frame error model on -------------------------------------------------------------------------------------

def test_error_model_verdicts_are_the_ones_counted(rsa, O):
    nd, lists, starts, air, want, _ = _batch_ref(True, R.SEED)
    plain = _batch_ref(True)[4]
    assert int(plain.t["rx_delivered"].sum()) - int(want.t["rx_delivered"].sum()) >= 50
    assert int(plain.t["tx_links_delivered"].sum()) - int(want.t["tx_links_delivered"].sum()) >= 50
    eng, dev = _engine(rsa, nd, em_seed=R.SEED), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        S.equal(eng.stats_read()[0], want, "batch with E10")
    finally:
        for d in dev:
            d.free()
        eng.close()
    nd, srcs, start, air = R.scene_lone()
    want, _ = _replay_table(nd, [srcs], [start], air, R.SEED)
    eng, d = _engine(rsa, nd, em_seed=R.SEED), DeviceArray(srcs)
    try:
        _lone(eng, "sources", d, srcs, start, air)
        S.equal(eng.stats_read()[0], want, "lone tick with E10")
    finally:
        d.free()
        eng.close()


# ---- 5. CSMA-CA: whole and split ------------------------------------------------------------------------------------------

def test_csma_whole_and_split_give_identical_tables(rsa, O):
    sc = BR.scene(O, "multi")
    n_ticks, p = SR.SCENES["multi"]
    r = SR.run(O, "multi")
    want = S.Table(sc.nd.n)
    for b in range(n_ticks):
        want.add_expected(r.exp[b], int(r.n_exp[b]))
    assert want.t["tx_frames"].sum() == int((r.status == SR.SENT).sum())
    t_cca = [sc.times(k)[1] for k in range(n_ticks)]
    tables = []
    for cuts in ((), (6,)):
        eng = _engine(rsa, sc.nd, sc.params)
        try:
            edges, carry = [0] + list(cuts) + [n_ticks], None
            for first, last in zip(edges[:-1], edges[1:]):
                want_carry, _ = KR.carry_at(r, first, t_cca)
                carry = want_carry[:0] if carry is None else carry
                _, _, _, carry = _part(rsa, eng, sc, r.lists[first:last], first, "device", sc.threshold, p, carry)
            tbl, tot = eng.stats_read()
            S.equal(tbl, want, "cuts %s" % (cuts,))
            assert int(tbl["tx_frames"].sum()) == int((r.status == SR.SENT).sum())
            assert tot["ticks_skipped"] == 0
            tables.append(tbl)
        finally:
            eng.close()
    np.testing.assert_array_equal(tables[0], tables[1])


# ---- 6. accumulation and control ------------------------------------------------------------------------------------------

def test_accumulation_and_control(rsa, O):
    nd, srcs, start, air = R.scene_lone()
    one, _ = _replay_table(nd, [srcs], [start], air)
    eng, d = _engine(rsa, nd, stats=False), DeviceArray(srcs)
    far = 100 * TICK   # (a later call starts after the frames of the one before have left the air)
    clock = [0]

    def tick():
        t = clock[0]
        clock[0] += far
        _lone(eng, "sources", d, srcs, t, air, t0=t)

    def times(k):
        w = S.Table(nd.n)
        for c in S.COLS:
            w.t[c] = one.t[c] * np.uint64(k)
        return w

    try:
        _refused(rsa, eng, STATE, eng.stats_read)            # before the first enable
        _refused(rsa, eng, STATE, eng.stats_device)
        _refused(rsa, eng, STATE, eng.stats_reset)
        tick()                                               # off: not counted
        eng.stats_enable()
        S.equal(eng.stats_read()[0], times(0), "fresh table")
        tick()
        tick()
        tbl, tot = eng.stats_read()
        S.equal(tbl, times(2), "two calls add up")
        assert tot == {"ticks_counted": 2, "ticks_skipped": 0}
        # a list read, the device pointers
        idx = np.array([int(srcs[3]), 0, nd.n - 1, int(srcs[0]), int(srcs[3])], dtype=np.int32)
        part, tot_l = eng.stats_read(idx)
        np.testing.assert_array_equal(part, tbl[idx])
        assert tot_l == tot
        big = np.random.default_rng(1).integers(0, nd.n, 5000).astype(np.int32)
        np.testing.assert_array_equal(eng.stats_read(big)[0], tbl[big])
        _refused(rsa, eng, INVALID, lambda: eng.stats_read(np.array([0, nd.n], dtype=np.int32)))
        _refused(rsa, eng, INVALID, lambda: eng.stats_read(np.array([-1], dtype=np.int32)))
        p_tbl, p_tot = eng.stats_device()
        np.testing.assert_array_equal(DeviceArray.read(p_tbl, rsa.NODE_STATS_DTYPE, nd.n), tbl)
        np.testing.assert_array_equal(DeviceArray.read(p_tot, np.uint64, 2), [2, 0])
        # off keeps the table, on goes on from it
        eng.stats_enable(False)
        assert not eng.stats_enabled()
        tick()
        S.equal(eng.stats_read()[0], times(2), "off: not counted, table kept")
        eng.stats_enable()
        tick()
        S.equal(eng.stats_read()[0], times(3), "on again")
        # the medium and the nodes may change: the counters stay
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
        eng.seed(3)
        i = int(srcs[0])
        eng.update_node(i, float(nd.x[i]), float(nd.y[i]), float(nd.z[i]), float(nd.txpower[i]), int(nd.channel[i]), 1, 1.0, 1.0)
        S.equal(eng.stats_read()[0], times(3), "rm_set_model / rm_seed / rm_node_update")
        tick()
        S.equal(eng.stats_read()[0], times(4), "counting goes on")
        eng.upload_table(nd)
        S.equal(eng.stats_read()[0], times(4), "rm_nodes_upload, same count")
        eng.stats_reset()
        tbl, tot = eng.stats_read()
        S.equal(tbl, times(0), "reset")
        assert tot == {"ticks_counted": 0, "ticks_skipped": 0}
        tick()
        S.equal(eng.stats_read()[0], times(1), "after reset")
        # another node count: resized and zeroed
        half = O.NodeTable(nd.n // 2)
        half.x, half.y = nd.x[:nd.n // 2], nd.y[:nd.n // 2]
        eng.upload_table(half)
        tbl, tot = eng.stats_read()
        assert len(tbl) == nd.n // 2 and not any(tbl[c].any() for c in S.COLS) and tot["ticks_counted"] == 0
        assert eng.stats_enabled()
    finally:
        d.free()
        eng.close()


# ---- 7. a skipped tick ----------------------------------------------------------------------------------------------------

def test_a_tick_over_the_link_capacity_is_skipped(rsa, O):
    """a self-contained batch of a tick of 150 frames and two ticks of three and two frames under a link capacity one below the large
    tick's link count (the sweep's candidate lists are sized by the capacity too, so the ticks that are to survive are small): the
    engine reports that slot as dropped and the other two as whole, and the table has exactly the other two"""
    nd, lists, starts, air = R.scene_batch(False)
    lists, starts = [lists[3], lists[4][:3], lists[5][:2]], starts[3:]
    _, res = _replay_table(nd, lists, starts, air)
    counts = [w.count for w in res]
    big, cap = 0, counts[0] - 1
    assert cap > 16384 and all(0 < 16 * c < cap for c in counts[1:])
    want = S.Table(nd.n)
    for k, (l, s, w) in enumerate(zip(lists, starts, res)):
        if k == big:
            want.skip()
        else:
            want.add_result(_packets(nd, l, s, air), w, verdict=w.plain)
    eng, dev = _engine(rsa, nd, cap=cap), []
    try:
        _run_batch(eng, lists, starts, air, dev)
        tbl, tot = eng.stats_read()
        print("heard and dropped per slot:", [eng.batch_result_count(k) for k in range(len(lists))], "totals:", tot)
        assert [bool(eng.batch_result_count(k)[1]) for k in range(len(lists))] == [k == big for k in range(len(lists))]
        S.equal(tbl, want, "batch with one dropped tick")
        assert tot == {"ticks_counted": len(lists) - 1, "ticks_skipped": 1}
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 8. off means off, on means one launch ----------------------------------------------------------------------------------

def _launches(eng):
    k = eng.profile_kernels()
    return {name: (v[0] if isinstance(v, (tuple, list)) else v) for name, v in k.items()}, list(k)


@pytest.mark.parametrize("mode", ["off", "on", "on+E10"])
def test_off_launches_nothing_and_on_launches_once_per_batch(rsa, O, mode):
    nd, lists, starts, air = R.scene_batch(True)
    lists = [l for l in lists if len(l)]
    starts = starts[:len(lists)]
    eng, dev = _engine(rsa, nd, stats=mode != "off", em_seed=R.SEED if mode == "on+E10" else None), []
    try:
        eng.profile_enable(1)
        _run_batch(eng, lists, starts, air, dev)
        eng.sync()
        n, order = _launches(eng)
        seen = {k: v for k, v in n.items() if k in STATS_KERNELS}
        assert seen == ({} if mode == "off" else {"k_stats_batch": 1}), (seen, order)
        if mode == "on+E10":
            assert n["k_errmodel_batch"] == 1 and order.index("k_errmodel_batch") < order.index("k_stats_batch"), order
        if mode != "off":
            _run_batch(eng, lists, [s + 50 * TICK for s in starts], air, dev)
            eng.sync()
            assert _launches(eng)[0]["k_stats_batch"] == 2
    finally:
        for d in dev:
            d.free()
        eng.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_window_and_table_unchanged(rsa, O):
    from radio_sim_amd import _lib
    nd, srcs, start, air = R.scene_lone()
    eng, d = _engine(rsa, nd), DeviceArray(srcs)
    clock, ticks = [0], [0]
    try:
        def plain(what):
            """a plain lone tick is the oracle's (the window is unharmed) and adds exactly one tick's worth to the table"""
            t = clock[0]
            clock[0] += 20 * TICK
            before = eng.stats_read()[0]
            w, _ = R.Replay(nd).tick(t, srcs, t, air)
            got = _lone(eng, "sources", d, srcs, t, air, t0=t)
            assert got.count == w.count, what
            np.testing.assert_array_equal(got.dst, w.dst, err_msg=what)
            np.testing.assert_array_equal(got.verdict, w.plain, err_msg=what)
            np.testing.assert_array_equal(_bits(got.sinr), _bits(w.sinr), err_msg=what)
            one = S.Table(nd.n)
            one.add_result(_packets(nd, srcs, t, air), w, verdict=w.plain)
            after, tot = eng.stats_read()
            ticks[0] += 1
            for c in S.COLS:
                np.testing.assert_array_equal(after[c] - before[c], one.t[c], err_msg="%s: %s" % (what, c))
            assert tot == {"ticks_counted": ticks[0], "ticks_skipped": 0}, what

        def refused(what, call, partition=None):
            t = clock[0]
            before = eng.stats_read()
            if partition:
                partition()
            _refused(rsa, eng, STATE, lambda: call(t))
            if partition:
                eng.set_partition(0, nd.n)
            after = eng.stats_read()
            np.testing.assert_array_equal(after[0], before[0], err_msg=what)
            assert after[1] == before[1], what
            plain(what)

        def flush(t):
            eng.tick_begin(t, t + TICK)
            eng.enqueue_tx(int(srcs[0]), t, air)
            eng.tick_flush(cap=1 << 16)

        plain("enabling")
        half = lambda: eng.set_partition(0, nd.n // 2)   # noqa: E731
        refused("a lone tick on a partition", lambda t: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air), half)
        refused("a lone tick on a spatial partition", lambda t: eng.tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air),
                lambda: eng.set_partition_spatial(0, 2))
        refused("a batch on a partition", lambda t: eng.batch_run_sources_device([t], [t + TICK], [d.ptr.value], [len(srcs)], [t], [air]), half)
        refused("rm_tick_flush on a partition", flush, half)
        refused("rm_transmit on a partition", lambda t: eng.transmit(int(srcs[0]), t, 254, cap=1 << 16), half)
        refused("gathered sources", lambda t: eng.batch_run_gathered_sources_device([t], [t + TICK], d.ptr.value, 1, len(srcs), [t], air))
        refused("rm_dist_batch", lambda t: eng.dist_batch_run_sources_device([t], [t + TICK], d.ptr.value, len(srcs), [t], air))
        refused("rm_dist_tick", lambda t: eng.dist_tick_run_sources_device(t, t + TICK, d.ptr.value, len(srcs), t, air))
        # a reference medium too (its ticks take other entry points)
        eng.set_model(1)
        eng.set_partition(0, nd.n // 2)
        _refused(rsa, eng, STATE, lambda: flush(clock[0]))
        _refused(rsa, eng, STATE, lambda: eng.tick_run_sources_device(clock[0], clock[0] + TICK, d.ptr.value, len(srcs), clock[0], air))
        _refused(rsa, eng, STATE, lambda: eng.transmit(int(srcs[0]), clock[0], 254, cap=1 << 16))
        eng.set_partition(0, nd.n)
        assert eng.stats_read()[1]["ticks_counted"] == ticks[0]
        # rm_group_*: a member with statistics refuses the group's tick; off again, the group's tick runs
        grp = rsa.Group([0])
        try:
            grp.upload_table(nd)
            grp.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in R.PARAMS.items()})
            L = _lib.lib()
            member = L.rm_group_context(grp._h, 0)
            assert L.rm_stats_enable(member, 1) == 0 and L.rm_stats_enabled(member) == 1
            recs = to_tx_records(rsa, nd.packets(srcs, 0, air))
            _refused(rsa, grp, STATE, lambda: grp.tick(recs, 0, TICK, cap=1 << 20))
            out = np.zeros(nd.n, dtype=rsa.NODE_STATS_DTYPE)
            tot = _lib.StatsTotals()
            assert L.rm_stats_read(member, None, nd.n, out.ctypes.data, C.byref(tot)) == 0
            assert not any(out[c].any() for c in S.COLS) and tot.ticks_counted == 0
            assert L.rm_stats_enable(member, 0) == 0
            w, _ = R.Replay(nd).tick(0, srcs, 0, air)
            got = grp.tick(recs, 0, TICK, cap=1 << 20)
            assert got.count == w.count
            np.testing.assert_array_equal(got.verdict, w.plain)
        finally:
            grp.close()
    finally:
        d.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
import radio_sim_amd as rsa
eng = rsa.Engine(0)
try:
    try:
        eng.stats_enable()
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        assert not eng.stats_enabled()
        eng.stats_enable(False)
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_enable_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs: the pass is not part of them"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)


# ---- 10. the reception stage behind a counted batch ---------------------------------------------------------------------------

def test_events_process_batch_after_a_counted_batch(rsa, O):
    nd, rng = R.nodes(1500, seed=8)
    lists = [np.sort(rng.choice(nd.n, 40, replace=False)).astype(np.int32) for _ in range(3)]
    starts = [0, TICK, 2 * TICK]
    want, _ = _replay_table(nd, lists, starts, 640)
    got = []
    for stats in (False, True):
        eng, dev = _engine(rsa, nd, stats=stats), []
        try:
            eng.set_time(0)
            eng.events_enable()
            _run_batch(eng, lists, starts, 640, dev)
            got.append(eng.events_process_batch([TICK, 2 * TICK, 3 * TICK]))
            if stats:
                S.equal(eng.stats_read()[0], want, "batch behind the reception stage")
        finally:
            for d in dev:
                d.free()
            eng.close()
    delivered = 0
    for a, b in zip(*got):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]))
        delivered += len(a[0])
    assert delivered > 500
