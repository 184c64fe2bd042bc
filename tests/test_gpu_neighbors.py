"""The neighbour query (rm_neighbors_*, rm_neighbors.hip) and rm_linkstats_watch_device on the GPU.
Expected rows come from the oracle through tests/neighbors_ref.py alone (tests/test_neighbors_ref.py holds the scenes' conditions
for that reference).  Every comparison is exact: equal integers, equal rssi bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linkstats_ref as LK
import neighbors_ref as N
from test_gpu_cca import _bits, _engine
from util import DeviceArray

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY, STATE = -1, -4, -5
DIRS = (N.HEARD_BY, N.HEARS)
TICK, AIR = 1000, 4256


def _nb_kernels(eng):
    return {k for k in eng.profile_kernels() if k.startswith("k_nb_")}


def _paths(eng):
    """which query kernels ran: {"boxes", "scan"}"""
    names = [k for k in _nb_kernels(eng) if k.startswith("k_nb_query")]
    return {"scan" if k.replace(" ", "").endswith("true>") else "boxes" for k in names}


def _device_query(eng, direction, K, nodes, n_rows, rssi=True, degree=True):
    """the device form into buffers filled with a pattern -> the outputs as the host form returns them"""
    peer = DeviceArray(np.full(n_rows * K, 0x5A5A5A5A, dtype=np.int32))
    dr = DeviceArray(np.full(n_rows * K, 7.0)) if rssi else None
    dd = DeviceArray(np.full(n_rows, 0x5A5A5A5A, dtype=np.int32)) if degree else None
    dn = DeviceArray(np.ascontiguousarray(nodes, dtype=np.int32)) if nodes is not None else None
    try:
        eng.neighbors_device(direction, K, peer.ptr.value, dr.ptr.value if dr else None, dd.ptr.value if dd else None,
                             dn.ptr.value if dn else None, n_rows if dn else None)
        eng.sync()
        out = {"peer": DeviceArray.read(peer.ptr.value, np.int32, n_rows * K).reshape(n_rows, K)}
        if rssi:
            out["rssi"] = DeviceArray.read(dr.ptr.value, np.float64, n_rows * K).reshape(n_rows, K)
        if degree:
            out["degree"] = DeviceArray.read(dd.ptr.value, np.int32, n_rows)
        return out
    finally:
        for d in (peer, dr, dd, dn):
            if d is not None:
                d.free()


# ---- 1. rows against the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(N.SCENES))
def test_rows_against_the_reference(rsa, O, name):
    """both directions, every K, the all-nodes and list forms, host and device, with rssi / degree NULL.  Tables of up to 64 nodes
    are not sorted (the whole-table scan); the larger ones walk the boxes."""
    nd, params, found = N.scene(name)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        rng = np.random.default_rng(11)
        some = rng.permutation(nd.n)[:max(1, nd.n // 3)].astype(np.int32)
        some = np.concatenate([some, some[:2]])   # (a node may be asked twice)
        for d in DIRS:
            for K in N.KS:
                what = "%s dir=%d K=%d" % (name, d, K)
                want = N.rows(nd, params, d, K, None, found[d])
                N.same(eng.neighbors(d, K), want, what + " all, host")
                part = N.rows(nd, params, d, K, some, found[d])
                N.same(eng.neighbors(d, K, nodes=some), part, what + " list, host")
                if K in (1, 8):
                    N.same(_device_query(eng, d, K, None, nd.n), want, what + " all, device")
                    N.same(_device_query(eng, d, K, some, len(some), rssi=False), part, what + " list, device, no rssi")
                    N.same(_device_query(eng, d, K, some, len(some), degree=False), part, what + " list, device, no degree")
                    N.same(eng.neighbors(d, K, nodes=some, fields=()), part, what + " list, host, peer alone")
        assert _paths(eng) == ({"scan"} if nd.n <= 64 else {"boxes"}), _nb_kernels(eng)
    finally:
        eng.close()


# ---- 2. against the engine itself --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n300_shadow", "n300_shadow_sinr", "n65"])
def test_heard_by_row_is_a_lone_tick(rsa, O, name):
    """the HEARD_BY row of j equals rm_neighbors_from_result of a lone rm_tick_run_sources_device([j]) on the same context, and
    degree is that tick's link count"""
    nd, params, found = N.scene(name)
    sp = N.special(nd)
    eng = _engine(rsa, nd, params)
    try:
        for k, j in enumerate((0, 5, nd.n // 2, sp["S"], sp["OFF"], sp["LOUD"], sp["LONE"])):
            d = DeviceArray(np.array([j], dtype=np.int32))
            t0 = 10 * AIR * k   # (every frame alone on the air)
            eng.tick_run_sources_device(t0, t0 + TICK, d.ptr.value, 1, t0, AIR)
            res = eng.result_copy(1, cap=nd.n)
            d.free()
            lone = rsa.Engine.neighbors_from_result(res, 16)
            got = eng.neighbors(N.HEARD_BY, 16, nodes=[j])
            np.testing.assert_array_equal(got["peer"], lone["peer"])
            np.testing.assert_array_equal(_bits(got["rssi"]), _bits(lone["rssi"]))
            assert got["degree"][0] == lone["degree"][0] == res.count == len(found[N.HEARD_BY][j])
    finally:
        eng.close()


# ---- 3. table sizes where the walk can go wrong ------------------------------------------------------------------------------

_LARGE = {}


def _large(n):
    if n not in _LARGE:
        nd, ask = N.large(n)
        _LARGE[n] = (nd, ask, {N.HEARD_BY: N.links(nd, N.SHADOW, N.HEARD_BY, ask), N.HEARS: N.links_hears_large(nd, N.SHADOW, ask)})
    return _LARGE[n]


@pytest.mark.parametrize("n", [1025, 65537])
def test_table_sizes(rsa, O, n):
    """List queries at the field's corners and centre (and the crafted nodes), shadowed medium.
    1025 nodes: two boxes of 1024 receivers, a last group of one receiver.
    65 537 nodes: the smallest table at which every loop of the query takes a second round -- 65 boxes of 1024 receivers (the walk
    takes 64 a round), k_nb_prep's 64 workgroups of 256 nodes a round (from 16 385 nodes), and, with 70 radios off, the list of
    them that a HEARS wave walks 64 a round."""
    nd, ask, found = _large(n)
    assert (np.asarray(nd.enabled) == 0).sum() > 64
    eng = _engine(rsa, nd, N.SHADOW)
    try:
        eng.profile_enable(1)
        for d in DIRS:
            for K in (2, 16):
                want = N.rows(nd, N.SHADOW, d, K, ask, found[d])
                assert (want[2] > K).any() and (want[2] < K).any()
                N.same(eng.neighbors(d, K, nodes=ask), want, "n=%d dir=%d K=%d" % (n, d, K))
        assert _paths(eng) == {"boxes"}
    finally:
        eng.close()


# ---- 4. every state of the table ---------------------------------------------------------------------------------------------

def _update(eng, nd, j, **kw):
    """rm_node_update of node j, mirrored in the reference's table"""
    for k, v in kw.items():
        getattr(nd, k)[j] = v
    eng.update_node(j, nd.x[j], nd.y[j], nd.z[j], nd.txpower[j], int(nd.channel[j]), int(nd.enabled[j]), nd.rxprob[j], nd.txprob[j])


def _check_all(eng, nd, params, what, K=4):
    for d in DIRS:
        N.same(eng.neighbors(d, K), N.rows(nd, params, d, K), "%s dir=%d" % (what, d))


def test_after_node_changes(rsa, O):
    """a node moved out of its group's box (rm_node_update, rm_nodes_move); one far node's txpower raised until it enters other
    nodes' HEARS rows; a radio switched off and on; another sensitivity; a node moved outside the fp32 frame (the frame grows with
    it: its slack passes the plan's limit and the whole-table scan answers)"""
    nd0, params, _ = N.scene("n300_shadow")
    nd, sp = N._copy(nd0), N.special(nd0)
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        _check_all(eng, nd, params, "before")
        _update(eng, nd, 3, x=nd.x[sp["S"]] + 2.0, y=nd.y[sp["S"]] + 1.0)      # from the field to the crafted nodes
        _check_all(eng, nd, params, "rm_node_update: moved far")
        nd.x[[10, 11]], nd.y[[10, 11]] = [nd.x[sp["LONE"]] + 10.0, -300.0], [nd.y[sp["LONE"]], -300.0]
        eng.move_nodes(np.array([10, 11], dtype=np.int32), nd.x[[10, 11]], nd.y[[10, 11]])
        _check_all(eng, nd, params, "rm_nodes_move")
        assert N.rows(nd, params, N.HEARS, 4, [sp["LONE"]])[2][0] == 1
        before = N.rows(nd, params, N.HEARS, 4)
        _update(eng, nd, sp["LONE"], txpower=75.0)                             # 5 km and more away: now heard by the crafted nodes
        after = N.rows(nd, params, N.HEARS, 4)
        assert (after[0] == sp["LONE"]).any(axis=1).sum() > (before[0] == sp["LONE"]).any(axis=1).sum() + 5
        _check_all(eng, nd, params, "txpower raised")
        _update(eng, nd, sp["A"], enabled=0)
        _update(eng, nd, sp["OFF"], enabled=1)
        _check_all(eng, nd, params, "radios switched")
        params2 = dict(params, ld_sensitivity_dbm=-88.5)
        eng.set_model(4, **{("flags" if k == "ld_flags" else k): v for k, v in params2.items()})
        _check_all(eng, nd, params2, "another sensitivity")
        assert _paths(eng) == {"boxes"}
        _update(eng, nd, 20, x=4.0e7, y=-3.0e7)
        _check_all(eng, nd, params2, "outside the fp32 frame")
        assert _paths(eng) == {"boxes", "scan"}
    finally:
        eng.close()


def test_unbounded_model(rsa, O):
    """exponent 0 on 200 nodes: no finite cut-off, every same-channel enabled receiver with rxprob > 0 is a link"""
    nd = N.rich(200, 13)
    params = {"ld_sigma_db": 0.0, "ld_exponent": 0.0}
    eng = _engine(rsa, nd, params)
    try:
        eng.profile_enable(1)
        for d in DIRS:
            want = N.rows(nd, params, d, 16)
            assert want[2].max() >= nd.n - 4
            N.same(eng.neighbors(d, 16), want, "unbounded dir=%d" % d)
        assert _paths(eng) == {"scan"}
    finally:
        eng.close()


def test_both_kernel_paths(rsa, O):
    """the same scene through the boxes and through the whole-table scan (a far node makes the fp32 frame too coarse for the boxes;
    it hears nobody and nobody hears it): equal bits, and rm_profile_kernels tells which ran"""
    nd0, params, found = N.scene("n300_shadow")
    nd = N._copy(nd0)
    sp = N.special(nd)
    out = {}
    for path in ("boxes", "scan"):
        eng = _engine(rsa, nd, params)
        try:
            eng.profile_enable(1)
            if path == "scan":
                _update(eng, nd, sp["LONE"], x=5.0e7, y=5.0e7)
            out[path] = [eng.neighbors(d, 8) for d in DIRS]
            assert _paths(eng) == {path}, _nb_kernels(eng)
            assert ("k_nb_prep" in _nb_kernels(eng))
        finally:
            eng.close()
    for d in DIRS:
        N.same(out["boxes"][d], N.rows(nd0, params, d, 8, None, found[d]), "boxes dir=%d" % d)
        for f in ("peer", "degree"):
            np.testing.assert_array_equal(out["boxes"][d][f], out["scan"][d][f])
        np.testing.assert_array_equal(_bits(out["boxes"][d]["rssi"]), _bits(out["scan"][d]["rssi"]))


# ---- 5. read-only ------------------------------------------------------------------------------------------------------------

def _same_result(a, b, what):
    assert a.count == b.count, (what, a.count, b.count)
    for f in ("pkt", "dst", "verdict", "pkt_interference", "pkt_offset"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg="%s: %s" % (what, f))
    np.testing.assert_array_equal(_bits(a.rssi), _bits(b.rssi), err_msg=what + ": rssi")
    np.testing.assert_array_equal(_bits(a.sinr), _bits(b.sinr), err_msg=what + ": sinr")


def _asker(a):
    def ask():
        for d in DIRS:
            a.neighbors(d, 8)
        a.neighbors(N.HEARS, 2, nodes=[1, 2, 3])
    return ask


def test_a_query_leaves_the_generator_alone(rsa, O):
    """a lone tick whose verdicts are drawn from java.util.Random (fractional rxprob) gives the same bits and leaves the same
    generator state with queries around it as on a context that never queried"""
    nd0, params, _ = N.scene("n300_shadow")
    nd = N._copy(nd0)
    nd.rxprob[::5] = 0.6
    a, b = _engine(rsa, nd, params, 1 << 20), _engine(rsa, nd, params, 1 << 20)
    srcs = np.arange(0, nd.n, 7, dtype=np.int32)
    d = DeviceArray(srcs)
    try:
        ask, out = _asker(a), []
        for e in (a, b):
            e.seed(9)
            if e is a:
                ask()
            s0 = e.rng_state
            e.tick_run_sources_device(0, TICK, d.ptr.value, len(srcs), 0, AIR)
            if e is a:
                ask()
            out.append((e.result_copy(len(srcs), cap=1 << 18), s0, e.rng_state))
        _same_result(out[0][0], out[1][0], "lone tick")
        assert out[0][1:] == out[1][1:] and out[0][1] != out[0][2]
        assert len(set(out[0][0].verdict.tolist())) == 2
    finally:
        d.free()
        a.close()
        b.close()


def test_a_query_changes_nothing(rsa, O):
    """a plain batch, a CSMA-CA batch and a channel-energy query on the SINR medium give the same bits with queries in front of
    them as on a context that never queried; E11 / E14 tables and E13's missed table are unchanged by a query"""
    nd, params, _ = N.scene("n300_shadow_sinr")
    a, b = _engine(rsa, nd, params, 1 << 20), _engine(rsa, nd, params, 1 << 20)
    keep = []
    try:
        rng = np.random.default_rng(2)
        lists = [np.sort(rng.choice(nd.n, 40, replace=False)).astype(np.int32) for _ in range(4)]
        starts = [TICK * k for k in range(4)]
        sched = np.zeros((nd.n, 3), dtype=np.int64)
        sched[::3] = (1000, 400, 500)   # (asleep when the frames of these ticks begin)
        rows = np.full((nd.n, 4), -1, dtype=np.int32)
        rows[:, 0] = (np.arange(nd.n) + 1) % nd.n
        for e in (a, b):
            e.stats_enable()
            e.listen_set(sched)
            e.linkstats_enable(4)
            e.linkstats_watch(rows)
        ask = _asker(a)

        def both(fn):
            ask()
            ra, rb = fn(a), fn(b)
            ask()
            return ra, rb

        def batch(e):
            arrs = [DeviceArray(s) for s in lists]
            keep.extend(arrs)
            e.batch_run_sources_device(starts, [t + TICK for t in starts], [x.ptr.value for x in arrs], [len(s) for s in lists], starts, [AIR] * 4)
            return [e.batch_result_copy(k, len(lists[k]), cap=1 << 18) for k in range(4)]

        for k, (x, y) in enumerate(zip(*both(batch))):
            _same_result(x, y, "batch slot %d" % k)
        ea, eb = both(lambda e: e.channel_energy(3 * TICK + 500, cca_threshold_dbm=-90.0))
        np.testing.assert_array_equal(_bits(ea[0]), _bits(eb[0]))
        np.testing.assert_array_equal(ea[1], eb[1])
        assert (ea[1] != 0).any()

        def csma(e):
            t0 = [30 * TICK + s for s in starts]
            return e.batch_run_sources_csma(t0, [t + TICK for t in t0], lists, t0, [AIR] * 4, t0, -85.0, rsa.Engine.csma_params(seed=3))

        (ca, na), (cb, nb) = both(csma)
        np.testing.assert_array_equal(na, nb)
        for f in ca:
            np.testing.assert_array_equal(np.asarray(ca[f]).view(np.uint8), np.asarray(cb[f]).view(np.uint8), err_msg="csma " + f)
        # the tables of E11, E13 and E14: the same on both contexts, and a query between two reads changes nothing

        def tables(e):
            return (e.stats_read()[0].tobytes(), e.stats_read()[1], e.listen_missed().tobytes(), e.linkstats_read()[0].tobytes(),
                    e.linkstats_read()[1], e.linkstats_peers().tobytes())

        ta = tables(a)
        ask()
        assert tables(a) == ta == tables(b)
        assert np.frombuffer(ta[3], dtype=LK.DTYPE)["heard"].sum() > 0 and np.frombuffer(ta[2], dtype=np.uint64).sum() > 0
    finally:
        for d in keep:
            d.free()
        a.close()
        b.close()


# ---- 6. refusals, each with nothing launched ---------------------------------------------------------------------------------

def _refused(eng, code, fn):
    with pytest.raises(Exception) as e:
        fn()
    assert getattr(e.value, "code", None) == code, e.value
    assert _nb_kernels(eng) == set(), _nb_kernels(eng)


def test_refusals(rsa, O):
    nd, params, _ = N.scene("n65")
    eng = _engine(rsa, nd, params)
    peer = DeviceArray(np.zeros(nd.n * 16, dtype=np.int32))
    try:
        eng.profile_enable(1)
        L, h = eng._L, eng._h
        q = lambda *a: rsa._lib.check(L.rm_neighbors_query_device(*a))
        _refused(eng, INVALID, lambda: q(None, 0, 4, None, nd.n, peer.ptr.value, None, None))
        _refused(eng, INVALID, lambda: q(h, 0, 4, None, nd.n, None, None, None))
        _refused(eng, INVALID, lambda: rsa._lib.check(L.rm_neighbors_query(h, 0, 4, None, nd.n, None, None, None)))
        for K in (0, -1, 17):
            _refused(eng, INVALID, lambda: eng.neighbors(N.HEARS, K))
            _refused(eng, INVALID, lambda: q(h, 1, K, None, nd.n, peer.ptr.value, None, None))
        for d in (-1, 2):
            _refused(eng, INVALID, lambda: eng.neighbors(d, 4))
        _refused(eng, INVALID, lambda: q(h, 0, 4, None, -1, peer.ptr.value, None, None))
        _refused(eng, INVALID, lambda: q(h, 0, 4, None, nd.n - 1, peer.ptr.value, None, None))
        _refused(eng, INVALID, lambda: q(h, 0, 4, None, nd.n + 1, peer.ptr.value, None, None))
        for bad in ([0, -1], [nd.n], [3, -2 ** 31]):
            _refused(eng, INVALID, lambda: eng.neighbors(N.HEARD_BY, 4, nodes=bad))
        _refused(eng, CAPACITY, lambda: q(h, 0, 16, peer.ptr.value, (1 << 23) + 1, peer.ptr.value, None, None))
        assert eng.neighbors(N.HEARS, 4, nodes=[])["peer"].shape == (0, 4) and _nb_kernels(eng) == set()   # n == 0 is RM_OK
        eng.tick_begin(0, TICK)
        _refused(eng, STATE, lambda: eng.neighbors(N.HEARS, 4))
        eng.enqueue_tx(1, 0, AIR)
        eng.tick_flush(cap=1 << 12)
        eng.set_partition(0, nd.n // 2)
        _refused(eng, STATE, lambda: eng.neighbors(N.HEARS, 4))
        eng.set_partition(0, nd.n)
        eng.set_partition_spatial(0, 2)
        _refused(eng, STATE, lambda: eng.neighbors(N.HEARD_BY, 4))
        eng.set_partition_spatial(0, 1)
        for kind in (0, 1, 2, 3):
            eng.set_model(kind)
            _refused(eng, STATE, lambda: eng.neighbors(N.HEARD_BY, 4))
        eng.set_model(4)
        assert eng.neighbors(N.HEARD_BY, 4)["peer"].shape == (nd.n, 4) and _nb_kernels(eng) != set()
    finally:
        peer.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
import numpy as np
import radio_sim_amd as rsa
eng = rsa.Engine(0)
try:
    eng.upload_nodes(np.zeros(4), np.arange(4.0))
    eng.set_model(4)
    eng.profile_enable(1)
    try:
        eng.neighbors(rsa.NB_HEARS, 2)
    except rsa.RadioMediumError as e:
        assert e.code == -5 and "RM_GRAPH" in str(e), e
        assert not [k for k in eng.profile_kernels() if k.startswith("k_nb_")]
        print("REFUSED")
    else:
        print("ACCEPTED")
finally:
    eng.close()
"""


def test_query_is_refused_under_graph_replay(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- replays its ticks from captured graphs"""
    env = dict(os.environ, RM_GRAPH="1")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip().splitlines()[-1] == "REFUSED", (p.stdout, p.stderr)


def test_device_list_entries_outside_the_table(rsa, O):
    """-1, n_nodes and INT32_MIN in a device list: rows of -1, degree 0, and the other rows intact"""
    nd, params, found = N.scene("n300")
    eng = _engine(rsa, nd, params)
    try:
        ask = np.array([7, -1, 8, nd.n, -2 ** 31, 299, 2 ** 31 - 1], dtype=np.int32)
        for d in DIRS:
            want = N.rows(nd, params, d, 4, ask, found[d])
            assert (want[0][[1, 3, 4, 6]] == -1).all() and (want[2][[1, 3, 4, 6]] == 0).all() and want[2][[0, 2]].min() > 0
            N.same(_device_query(eng, d, 4, ask, len(ask)), want, "dir=%d" % d)
    finally:
        eng.close()


# ---- 7. the chain into E14 ---------------------------------------------------------------------------------------------------

def test_chain_into_watched_links(rsa, O):
    """neighbors_device(NB_HEARS, 4) -> linkstats_watch_device of that buffer -> a batch: peers and statistics equal those of a
    second context given the same rows through the host's linkstats_watch"""
    nd, params, found = N.scene("n300_shadow_sinr")
    a, b = _engine(rsa, nd, params, 1 << 20), _engine(rsa, nd, params, 1 << 20)
    peer = DeviceArray(np.zeros(nd.n * 4, dtype=np.int32))
    keep = [peer]
    try:
        want = N.rows(nd, params, N.HEARS, 4, None, found[N.HEARS])
        for e in (a, b):
            e.linkstats_enable(4)
        a.neighbors_device(N.HEARS, 4, peer.ptr.value)
        a.linkstats_watch_device(peer.ptr.value)
        b.linkstats_watch(want[0])
        np.testing.assert_array_equal(a.linkstats_peers(), want[0])
        rng = np.random.default_rng(4)
        lists = [np.sort(rng.choice(nd.n, 60, replace=False)).astype(np.int32) for _ in range(4)]
        t0 = [TICK * k for k in range(4)]
        for e in (a, b):
            arrs = [DeviceArray(s) for s in lists]
            keep.extend(arrs)
            e.batch_run_sources_device(t0, [t + TICK for t in t0], [x.ptr.value for x in arrs], [len(s) for s in lists], t0, [AIR] * 4)
        ta, tb = a.linkstats_read(), b.linkstats_read()
        assert ta[0].tobytes() == tb[0].tobytes() and ta[1] == tb[1] and ta[0]["heard"].sum() > 50
        np.testing.assert_array_equal(a.linkstats_peers(), b.linkstats_peers())
        # a list form: two nodes' rows replaced on the device, the others keep peers and history
        sub = np.array([5, 200], dtype=np.int32)
        new = np.full((2, 4), -1, dtype=np.int32)
        new[0, :2], new[1, 1] = (want[0][5, 1], 9), want[0][200, 1]
        dn, dp = DeviceArray(sub), DeviceArray(new)
        keep.extend([dn, dp])
        a.linkstats_watch_device(dp.ptr.value, dn.ptr.value, 2)
        b.linkstats_watch(new, nodes=sub)
        np.testing.assert_array_equal(a.linkstats_peers(), b.linkstats_peers())
        np.testing.assert_array_equal(a.linkstats_peers(nodes=sub), new)
        assert a.linkstats_read()[0].tobytes() == b.linkstats_read()[0].tobytes()
        # a host list watch after a device watch starts from the device's rows
        a.linkstats_watch(new[::-1].copy(), nodes=sub)
        b.linkstats_watch(new[::-1].copy(), nodes=sub)
        np.testing.assert_array_equal(a.linkstats_peers(), b.linkstats_peers())
        assert a.linkstats_read()[0].tobytes() == b.linkstats_read()[0].tobytes()
    finally:
        for d in keep:
            d.free()
        a.close()
        b.close()


def test_watch_device_refusals(rsa, O):
    """a duplicate in a row, an own-node entry, an out-of-range entry, a node listed twice or outside the table: RM_ERR_INVALID,
    peers and entries unchanged; RM_ERR_STATE while E14 is off"""
    nd, params, found = N.scene("n300_shadow_sinr")
    eng = _engine(rsa, nd, params, 1 << 20)
    keep = []

    def dev(a, dt=np.int32):
        d = DeviceArray(np.ascontiguousarray(a, dtype=dt))
        keep.append(d)
        return d.ptr.value

    try:
        good = N.rows(nd, params, N.HEARS, 4, None, found[N.HEARS])[0]
        with pytest.raises(rsa.RadioMediumError) as e:
            eng.linkstats_watch_device(dev(good))
        assert e.value.code == STATE
        eng.linkstats_enable(4)
        eng.linkstats_watch_device(dev(good))
        lists = [np.arange(0, nd.n, 3, dtype=np.int32)]
        eng.batch_run_sources_device([0], [TICK], [dev(lists[0])], [len(lists[0])], [0], [AIR])
        before = (eng.linkstats_peers().tobytes(), eng.linkstats_read()[0].tobytes())
        assert eng.linkstats_read()[0]["heard"].sum() > 0
        cases = []
        for j, k, v in ((17, 2, None), (40, 0, 40), (41, 3, nd.n), (42, 1, -2), (299, 3, 2 ** 31 - 1)):
            rows = good.copy()
            rows[j, k] = rows[j, (k + 1) % 4] if v is None else v
            if v is None:
                assert rows[j, k] >= 0   # (a duplicate of a real peer)
            cases.append((dev(rows), None, nd.n))
        cases.append((dev(good[:3]), dev([4, 9, 4]), 3))
        cases.append((dev(good[:3]), dev([4, -1, 5]), 3))
        cases.append((dev(good[:3]), dev([4, nd.n, 5]), 3))
        cases.append((dev(good), None, nd.n - 1))
        for rows_ptr, nodes_ptr, n in cases:
            with pytest.raises(rsa.RadioMediumError) as e:
                rsa._lib.check(eng._L.rm_linkstats_watch_device(eng._h, nodes_ptr, n, rows_ptr))
            assert e.value.code == INVALID
            assert (eng.linkstats_peers().tobytes(), eng.linkstats_read()[0].tobytes()) == before
        eng.linkstats_watch_device(dev(good[[9, 4]]), dev([9, 4]), 2)   # a valid list after the refused ones
    finally:
        for d in keep:
            d.free()
        eng.close()
