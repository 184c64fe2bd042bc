"""The link estimator (rm_linkest_*, rm_linkest.hip) on the GPU.  The scenes are those of
tests/linkest_ref.py -- tests/test_linkest_ref.py holds their conditions for the reference alone -- uploaded as explicit inputs, and
a chain over the context's own tables on the SINR medium; after EVERY fold the entries, the node state, the published peers and
entries and the totals are compared with the reference, bit for bit.  Host and device forms are used in turn."""
import ctypes as C

import numpy as np
import pytest

import linkest_ref as R
import nbtable_ref as NB
from test_gpu_fwd import launches_added
from util import DeviceArray, KINDS, _PARAM_MAP

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5
TICK, AIR = NB.TICK, NB.AIR


def _code(rsa, call):
    with pytest.raises(rsa.RadioMediumError) as e:
        call()
    return e.value.code


def read_all(eng, n, K):
    """the five tables: entries, node state, published peers and entries, totals"""
    ent, nod, tot = eng.linkest_read()
    peer_ptr, stats_ptr, k = eng.linkest_tables()
    assert k == K and ent.shape == (n, K)
    pub_peer = DeviceArray.read(peer_ptr, np.int32, n * K).reshape(n, K)
    pub_stats = DeviceArray.read(stats_ptr, R.LINK_STATS, n * K).reshape(n, K)
    return ent, nod, pub_peer, pub_stats, tot


def same(eng, ref, what):
    got = read_all(eng, ref.n, ref.K)
    R.same(ref, *got, what)
    return got


def bare(rsa, n):
    eng = rsa.Engine(0)
    eng.upload_table(NB.line_nodes(n))
    return eng


# ---- explicit inputs: the scenes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 9, 65, 257])
def test_explicit_input_folds(rsa, n, K):
    """n * K lanes: a wave's tail (1, 2, 3, 9 nodes), a second partial wave (9 x 8, 65 x 1), several workgroups (65 x 8, 257 x 1
    and up), single-row tables; the device form and the host form in turn, every third fold without the forwarding table"""
    eng = bare(rsa, n)
    bufs = []
    try:
        eng.linkest_enable(K)
        same(eng, R.Ref(n, K, R.params()), "after enable")
        ref = R.Ref(n, K, R.params())
        for f, (peer, stats, fwd) in enumerate(R.scene(n, K)):
            fw = None if f % 3 == 2 else fwd
            if f % 2:
                d = [DeviceArray(peer), DeviceArray(stats), None if fw is None else DeviceArray(fw)]
                bufs += [b for b in d if b is not None]
                eng.linkest_fold_device((d[0].ptr.value, d[1].ptr.value, None if fw is None else d[2].ptr.value, K))
            else:
                eng.linkest_fold(peer, stats, fw)
            ref.fold(peer, stats, fw)
            same(eng, ref, "n %d K %d fold %d" % (n, K, f))
        # a list read gives the listed rows in list order
        nodes = [n - 1, 0, n // 2]
        ent, nod, tot = eng.linkest_read(nodes)
        assert ent.tobytes() == ref.entry[nodes].tobytes() and nod.tobytes() == ref.node[nodes].tobytes() and tot == ref.totals()
        # reset: everything as after enable
        eng.linkest_reset()
        same(eng, R.Ref(n, K, R.params()), "after reset")
    finally:
        for b in bufs:
            b.free()
        eng.close()


@pytest.mark.parametrize("p", [R.params(beacon_window=1, data_window=1, beacon_alpha_q8=0, data_alpha_q8=255, max_etx=65535),
                               R.params(beacon_window=0), R.params(data_window=0, max_etx=128)])
def test_other_parameters(rsa, p):
    n, K = 65, 4
    eng = bare(rsa, n)
    try:
        eng.linkest_enable(K, **p)
        ref = R.Ref(n, K, p)
        for f, (peer, stats, fwd) in enumerate(R.scene(n, K, seed=7)):
            eng.linkest_fold(peer, stats, fwd)
            ref.fold(peer, stats, fwd)
            same(eng, ref, "fold %d" % f)
    finally:
        eng.close()


# ---- the context's own tables -------------------------------------------------------------------------------------------------------

SIDE = 8
ROOT = 27


def lattice_engine(rsa):
    """64 nodes 30 m apart on the SINR medium (capture at -1 dB): 20 neighbours in reach, neighbours that send together collide"""
    nd = NB.lattice_nodes(SIDE, 30.0)
    eng = rsa.Engine(0)
    eng.upload_table(nd)
    eng.set_model(KINDS["logdist"], **{_PARAM_MAP[k]: v for k, v in NB.LATTICE.items()})
    return eng, nd


def beacon_lists(n):
    """a cycle of twenty ticks: sixteen in which the nodes of one class (x mod 4, y mod 4) send -- senders four pitches apart, out
    of each other's receivers' reach: in the clear --, then the even, the odd, the even and the odd nodes (the neighbours left
    and right and above and below send together: collisions) -- a node sends three times per cycle, once in the clear"""
    j = np.arange(n)
    cls = (j % SIDE) % 4 + 4 * ((j // SIDE) % 4)
    clear = [j[cls == c].astype(np.int32) for c in range(16)]
    half = [np.arange(r, n, 2, dtype=np.int32) for r in range(2)]
    return [(DeviceArray(a), len(a)) for a in clear + half + half]


def lattice_watch(n, K, shift=0):
    """row j: the neighbours right, below, left, above (where they exist), then two and three to the right"""
    rows = np.full((n, K), -1, dtype=np.int32)
    for j in range(n):
        x, y = j % SIDE, j // SIDE
        near = [(x + 1, y), (x, y + 1), (x - 1, y), (x, y - 1), (x + 2, y), (x + 3, y), (x, y + 2), (x, y + 3)]
        peers = [b * SIDE + a for a, b in near if 0 <= a < SIDE and 0 <= b < SIDE]
        peers = peers[shift:] + peers[:shift]
        rows[j, :min(K, len(peers))] = peers[:K]
    return rows


def beacons(eng, src_bufs, t, rounds):
    """`rounds` ticks of the cycle, which goes on from tick to tick"""
    for r in range(rounds):
        d = src_bufs[(t // TICK) % len(src_bufs)]
        eng.tick_run_sources_device(t, t + TICK, d[0].ptr.value, d[1], t + 100, AIR)
        t += TICK
    return t


def test_own_table_chain(rsa):
    """E14 watch, ticks, a fold, six times and more -- with a watch change and rm_linkstats_reset on the way --, then E19 traffic
    along measured routes with an advance and a fold per tick: equal to the reference fed the tables read back"""
    K = 4
    eng, nd = lattice_engine(rsa)
    n = nd.n
    src = beacon_lists(n)
    d_src, d_count = DeviceArray(np.full(n, -1, dtype=np.int32)), DeviceArray(np.zeros(1, dtype=np.int32))
    try:
        eng.linkstats_enable(K)
        eng.linkstats_watch(lattice_watch(n, K))
        p = R.params(beacon_window=2, data_window=2)
        eng.linkest_enable(K, **p)
        ref = R.Ref(n, K, p)
        t = 0

        def fold(what, device):
            fwd = eng.fwd_read()[0] if eng.fwd_enabled() else None
            peers, stats = eng.linkstats_peers(), eng.linkstats_read()[0]
            if device:
                eng.linkest_fold_device(None)
            else:
                eng.linkest_fold()
            ref.fold(peers, stats.astype(R.LINK_STATS), None if fwd is None else fwd.astype(R.FWD_NODE))
            same(eng, ref, what)
            # E14's and E19's tables are not written
            assert eng.linkstats_peers().tobytes() == peers.tobytes() and eng.linkstats_read()[0].tobytes() == stats.tobytes()
            assert fwd is None or eng.fwd_read()[0].tobytes() == fwd.tobytes()
        for step in range(8):
            if step == 3:
                eng.linkstats_watch(lattice_watch(n, K, shift=1)[::2], nodes=list(range(0, n, 2)))   # (every other row: restarts)
            if step == 5:
                eng.linkstats_reset()                                                                  # (every counter shrinks)
            t = beacons(eng, src, t, 10)
            fold("beacon step %d" % step, step % 2 == 1)
        tot = ref.totals()
        print("chain, beacons:", tot, dict(ref.log))
        assert tot["beacon_samples"] >= n and tot["restarted"] >= 2 * n and ref.log["partial"] >= 1 and ref.log["between_seen"] >= 1
        assert ref.log["zero_delivered"] >= 1 and tot["data_samples"] == 0                          # (collisions; no E19 yet)
        # E19: routes over the smoothed costs, then traffic toward the root
        out, rt = eng.etx_routes(eng.etx_params(min_heard=1, max_link_cost=6000), [ROOT], tables=read_all(eng, n, K)[2:4])
        assert rt["reached"] >= 2                    # (somebody has a route: there is traffic to forward)
        eng.fwd_enable(queue_slots=4)
        eng.fwd_set_next(out["parent"], [ROOT], t)
        for step in range(10):
            eng.fwd_inject(list(range(n)), t)
            eng.fwd_sources_device(t + 100, n, d_src.ptr.value, d_count.ptr.value)
            eng.tick_run_sources_device(t, t + TICK, d_src.ptr.value, n, t + 100, AIR)
            eng.fwd_advance_device(0, None, 0)
            t += TICK
            fold("data step %d" % step, step % 2 == 0)
        tot = ref.totals()
        print("chain, data:", tot, dict(ref.log), rt)
        assert tot["data_samples"] >= 4 and int(ref.entry["data_windows"].sum()) >= 4
    finally:
        for d, _ in src:
            d.free()
        d_src.free()
        d_count.free()
        eng.close()


# ---- the measured-route query over the published table ------------------------------------------------------------------------------

def _routes_device(eng, n, P, tables, roots):
    bufs = [DeviceArray(np.asarray(roots, dtype=np.int32)), DeviceArray(nbytes=8 * n), DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n),
            DeviceArray(nbytes=4 * n)]
    try:
        tot = eng.etx_routes_device(P, bufs[0].ptr.value, len(roots), bufs[1].ptr.value, bufs[2].ptr.value, bufs[3].ptr.value, bufs[4].ptr.value,
                                    dev_tables=tables)
        return (DeviceArray.read(bufs[1].ptr.value, np.uint64, n), DeviceArray.read(bufs[2].ptr.value, np.int32, n),
                DeviceArray.read(bufs[3].ptr.value, np.int32, n), DeviceArray.read(bufs[4].ptr.value, np.uint32, n), tot)
    finally:
        for b in bufs:
            b.free()


def test_routes_over_the_published_table(rsa):
    """rm_etx_query_device over rm_linkest_tables equals rm_etx_from_tables over the published table read back; and after one fold
    from reset with alpha 0, no data samples and beacon_window W it equals E21 over E14's own tables with min_heard W and a
    max_link_cost below max_etx (an entry without a delivery is published at max_etx, which the cap then leaves out as E21 leaves
    out delivered == 0; whether the run holds such an entry is the medium's doing and is printed, not asserted)"""
    K, W = 4, 4
    eng, nd = lattice_engine(rsa)
    n = nd.n
    src = beacon_lists(n)
    try:
        eng.linkstats_enable(K)
        eng.linkstats_watch(lattice_watch(n, K))
        eng.linkest_enable(K, beacon_window=W, data_window=0, beacon_alpha_q8=0, max_etx=6400)
        t = beacons(eng, src, 0, 20)
        eng.linkest_fold()
        t = beacons(eng, src, t, 20)
        eng.linkest_fold()
        for hyst in (0, 192):
            P = eng.etx_params(min_heard=1, max_link_cost=2048, hysteresis=hyst)
            pub = read_all(eng, n, K)[2:4]
            print("routes: published", np.unique(pub[1]["heard"], return_counts=True))
            assert (pub[1]["heard"] > 128).any()
            got = _routes_device(eng, n, P, eng.linkest_tables(), [ROOT, 5])
            want, wt = eng.etx_from_tables(pub, P, [ROOT, 5])
            assert got[4] == wt and wt["reached"] >= 2
            for a, f in zip(got[:4], ("cost", "parent", "slot", "link_cost")):
                assert a.tobytes() == want[f].tobytes(), f
        # one fold from reset: the raw window
        eng.linkest_reset()
        eng.linkest_fold_device(None)
        stats = eng.linkstats_read()[0]
        print("routes: heard", np.unique(stats["heard"], return_counts=True), "delivered", np.unique(stats["delivered"], return_counts=True))
        assert (stats["heard"] >= W).any()
        own = _routes_device(eng, n, eng.etx_params(min_heard=W, max_link_cost=2048, hysteresis=0), None, [ROOT])
        pub = _routes_device(eng, n, eng.etx_params(min_heard=1, max_link_cost=2048, hysteresis=0), eng.linkest_tables(), [ROOT])
        assert own[4] == pub[4] and own[4]["reached"] >= 2
        for a, b, f in zip(own[:4], pub[:4], ("cost", "parent", "slot", "link_cost")):
            assert a.tobytes() == b.tobytes(), f
    finally:
        for d, _ in src:
            d.free()
        eng.close()


def test_cap_leaves_out_an_entry_without_a_delivery(rsa):
    """explicit inputs that pin the exclusion: a slot with H >= W and D == 0 is published at max_etx, which a max_link_cost below
    max_etx leaves out exactly as E21 leaves out delivered == 0 over the raw table; a slot with H < W has no estimate and is left
    out as min_heard = W leaves it out.  Node 1 hears only node 0 and never a delivery, node 2 hears 0 (4 of 8) and 1 (8 of 8),
    node 3 hears node 2 twice (below W)"""
    n, K, W = 4, 2, 4
    peer = np.array([[-1, -1], [0, -1], [0, 1], [2, -1]], dtype=np.int32)
    stats = R.cleared_stats((n, K))
    for (j, k), (h, d) in {(1, 0): (8, 0), (2, 0): (8, 4), (2, 1): (8, 8), (3, 0): (2, 2)}.items():
        stats[j, k]["heard"], stats[j, k]["delivered"] = h, d
    eng = bare(rsa, n)
    try:
        eng.linkest_enable(K, beacon_window=W, data_window=0, beacon_alpha_q8=0, max_etx=6400)
        eng.linkest_fold(peer, stats, None)
        ent, _, pub_peer, pub_stats, tot = read_all(eng, n, K)
        assert ent["etx"].tolist() == [[0, 0], [6400, 0], [256, 128], [0, 0]] and tot["estimates"] == 3
        assert pub_stats["heard"].tolist() == ent["etx"].tolist() and pub_peer.tolist() == peer.tolist()
        raw, rt = eng.etx_routes(eng.etx_params(min_heard=W, max_link_cost=2048, hysteresis=0), [0], tables=(peer, stats))
        got = _routes_device(eng, n, eng.etx_params(min_heard=1, max_link_cost=2048, hysteresis=0), eng.linkest_tables(), [0])
        unreached = (1 << 64) - 1
        assert got[0].tolist() == [0, unreached, 256, unreached] and got[1].tolist() == [-1, -1, 0, -1]
        assert got[4] == rt and rt["reached"] == 2
        for a, f in zip(got[:4], ("cost", "parent", "slot", "link_cost")):
            assert a.tobytes() == raw[f].tobytes(), f
        # with the cap at max_etx the entry counts: the exclusion above is the cap's doing
        got = _routes_device(eng, n, eng.etx_params(min_heard=1, max_link_cost=6400, hysteresis=0), eng.linkest_tables(), [0])
        assert got[0].tolist() == [0, 6400, 256, unreached]
    finally:
        eng.close()


# ---- E22 beside it --------------------------------------------------------------------------------------------------------------------

def test_neighbour_tables_are_the_same_with_folds(rsa):
    """rm_nbtable_update and rm_nbtable_expire after folds give what they give without the estimator: it writes none of E14's
    tables and needs no rm_linkstats_reset"""
    K = 4
    outs = []
    for with_est in (False, True):
        eng, nd = lattice_engine(rsa)
        n = nd.n
        src = [(DeviceArray(np.arange(r, n, 3, dtype=np.int32)), len(range(r, n, 3))) for r in range(3)]
        try:
            eng.linkstats_enable(K)
            eng.nbtable_enable(timeout_us=4 * TICK, evict_cost=300, min_heard=2, admit_rssi_dbm=-92.0)
            if with_est:
                eng.linkest_enable(K, beacon_window=2)
            t = 0
            for step in range(12):
                d = src[0 if step >= 5 else step % 3]     # (from step 5 on two thirds of the nodes are silent: stale slots)
                eng.tick_run_sources_device(t, t + TICK, d[0].ptr.value, d[1], t + 100, AIR)
                t += TICK
                eng.nbtable_update(0, t)
                if with_est:
                    eng.linkest_fold_device(None)
                if step == 9:
                    eng.nbtable_expire(t)
                    if with_est:
                        eng.linkest_fold()
            rows, tot = eng.nbtable_read()
            outs.append((eng.linkstats_peers().tobytes(), eng.linkstats_read()[0].tobytes(), rows.tobytes(), tot))
            assert tot["admitted"] >= n // 4 and tot["evicted_stale"] + tot["evicted_poor"] + tot["expired"] >= 1
            if with_est:
                lt = eng.linkest_read()[2]
                assert lt["folds"] == 13 and lt["restarted"] >= n // 4 and lt["beacon_samples"] >= 1
        finally:
            for d, _ in src:
                d.free()
            eng.close()
    assert outs[0] == outs[1]


# ---- one launch; off by default -----------------------------------------------------------------------------------------------------

def test_one_launch_per_fold_and_nothing_while_off(rsa):
    eng, nd = lattice_engine(rsa)
    n = nd.n
    src = DeviceArray(np.arange(0, n, 3, dtype=np.int32))
    try:
        eng.profile_enable(1)
        eng.linkstats_enable(4)
        eng.linkstats_watch(lattice_watch(n, 4))
        eng.fwd_enable()
        assert eng.linkest_enabled() == 0
        eng.tick_run_sources_device(0, TICK, src.ptr.value, len(range(0, n, 3)), 100, AIR)
        eng.fwd_advance(0)
        eng.etx_routes(eng.etx_params(min_heard=1), [ROOT])
        assert not [k for k in eng.profile_kernels() if k.startswith("k_lest_")]
        assert _code(rsa, lambda: eng.linkest_fold()) == STATE
        assert not [k for k in eng.profile_kernels() if k.startswith("k_lest_")]
        eng.linkest_enable(4)
        assert eng.linkest_enabled() == 4
        added = launches_added(eng, "k_lest_", lambda: eng.linkest_fold())
        assert added == {"k_lest_fold": 1}, added
        peer, stats = eng.linkstats_peers(), eng.linkstats_read()[0]
        added = launches_added(eng, "k_lest_", lambda: eng.linkest_fold(peer, stats, eng.fwd_read()[0]))
        assert added == {"k_lest_fold": 1}, added
        assert eng.linkest_read()[2]["folds"] == 2
    finally:
        src.free()
        eng.close()


# ---- refusals and lifetime ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_tables_untouched(rsa):
    n, K = 9, 2
    eng = bare(rsa, n)
    seq = R.scene(n, K)
    bufs = []
    try:
        L, h = eng._L, eng._h
        I = rsa._lib.LinkEstInputs
        good = eng.linkest_params()
        # off: every call but enable / enabled / disable is STATE, and arguments are checked before state
        for call in (lambda: eng.linkest_fold(), lambda: eng.linkest_fold_device(None), lambda: eng.linkest_read(), lambda: eng.linkest_reset(),
                     lambda: eng.linkest_device(), lambda: eng.linkest_tables(), lambda: eng.linkest_get_params()):
            assert _code(rsa, call) == STATE
        assert L.rm_linkest_fold(h, C.byref(I(peer=None, stats=None, fwd=None, K=K, reserved=0))) == INVALID
        eng.linkest_disable()
        # enable: INVALID before anything changes
        for kw in (dict(beacon_window=(1 << 31) + 1), dict(data_window=(1 << 31) + 1), dict(beacon_alpha_q8=256), dict(data_alpha_q8=256),
                   dict(max_etx=127), dict(max_etx=65536), dict(reserved=1)):
            bad = eng.linkest_params(**kw)
            assert _code(rsa, lambda: eng.linkest_enable(K, bad)) == INVALID and eng.linkest_enabled() == 0
        for k in (0, 3, 5, 16, -1):
            assert _code(rsa, lambda: eng.linkest_enable(k)) == INVALID
        assert L.rm_linkest_enable(h, K, None) == INVALID and L.rm_linkest_enable(None, K, C.byref(good)) == INVALID
        eng.linkest_enable(K)
        ref = R.Ref(n, K, R.params())
        for peer, stats, fwd in seq[:6]:
            eng.linkest_fold(peer, stats, fwd)
            ref.fold(peer, stats, fwd)
        same(eng, ref, "before the refusals")
        peer, stats, fwd = seq[6]
        d = [DeviceArray(peer), DeviceArray(stats), DeviceArray(fwd)]
        bufs += d
        dp, ds, df = (b.ptr.value for b in d)
        ok = dict(peer=dp, stats=ds, fwd=df, K=K, reserved=0)
        # INVALID: explicit inputs with another K, a reserved field, a NULL or misaligned peer or stats
        for kw in (dict(K=4), dict(K=3), dict(K=0), dict(reserved=1), dict(peer=None), dict(stats=None), dict(peer=dp + 4), dict(stats=ds + 4),
                   dict(fwd=df + 4)):
            f = dict(ok)
            f.update(kw)
            assert L.rm_linkest_fold_device(h, C.byref(I(**f))) == INVALID, kw
        hp = dict(peer=peer.ctypes.data, stats=stats.ctypes.data, fwd=fwd.ctypes.data, K=K, reserved=0)
        for kw in (dict(K=4), dict(reserved=1), dict(peer=None), dict(stats=None)):
            f = dict(hp)
            f.update(kw)
            assert L.rm_linkest_fold(h, C.byref(I(**f))) == INVALID, kw
        assert L.rm_linkest_fold(None, None) == INVALID and L.rm_linkest_fold_device(None, None) == INVALID
        assert L.rm_linkest_read(h, None, 3, None, None, None) == INVALID and L.rm_linkest_read(h, None, -1, None, None, None) == INVALID
        assert L.rm_linkest_read(h, np.array([n], dtype=np.int32).ctypes.data, 1, None, None, None) == INVALID
        assert L.rm_linkest_get_params(h, None) == INVALID and L.rm_linkest_tables(h, None) == INVALID and L.rm_linkest_reset(None) == INVALID
        same(eng, ref, "after the INVALID refusals")
        # STATE: own tables while E14 is off or has another K; a receiver partition; inside an open tick
        assert _code(rsa, lambda: eng.linkest_fold()) == STATE and _code(rsa, lambda: eng.linkest_fold_device(None)) == STATE
        eng.linkstats_enable(4)
        assert _code(rsa, lambda: eng.linkest_fold()) == STATE
        eng.linkstats_enable(K)
        eng.linkest_fold_device(None)                     # (the same K: accepted; every slot of the fresh watch table is empty)
        ref.fold(np.full((n, K), -1, dtype=np.int32), R.cleared_stats((n, K)), None)
        same(eng, ref, "an own-table fold over an empty watch table")
        eng.linkstats_enable(4)                           # (another K: the feature stays on, own-table folds are refused)
        assert eng.linkest_enabled() == K and _code(rsa, lambda: eng.linkest_fold()) == STATE
        eng.linkest_fold(peer, stats, fwd)                # (explicit inputs are still taken)
        ref.fold(peer, stats, fwd)
        eng.set_partition(0, n // 2)
        assert _code(rsa, lambda: eng.linkest_fold(peer, stats, fwd)) == STATE
        assert L.rm_linkest_fold_device(h, C.byref(I(**ok))) == STATE
        assert _code(rsa, lambda: eng.linkest_enable(K)) == STATE and eng.linkest_enabled() == K
        eng.set_partition(0, n)
        eng.tick_begin(0, TICK)
        assert _code(rsa, lambda: eng.linkest_fold(peer, stats, fwd)) == STATE
        assert L.rm_linkest_fold_device(h, C.byref(I(**ok))) == STATE
        eng.enqueue_tx(1, 0, AIR)
        eng.tick_flush(cap=1 << 12)
        same(eng, ref, "after the STATE refusals")
        # rm_node_update, rm_nodes_move, rm_set_model, rm_seed and the same node count keep everything
        nd = NB.line_nodes(n)
        eng.upload_table(nd)
        eng.update_node(1, 1.0, 0.0, 0.0, 0.0, int(nd.channel[1]), 1, 1.0, 1.0)
        eng.move_nodes([2, 3], [0.5, 1.5], [0.0, 0.0])
        eng.set_model(KINDS["udgm"])
        eng.seed(7)
        same(eng, ref, "after an upload of the same node count, an update, a move, a model and a seed")
        assert eng.linkest_get_params().max_etx == 6400 and all(eng.linkest_device()) and all(eng.linkest_tables())
        # enable again: anew, with the new K
        eng.linkest_enable(4, max_etx=500)
        same(eng, R.Ref(n, 4, R.params(max_etx=500)), "after another enable")
        assert eng.linkest_get_params().max_etx == 500
        # another node count switches it off
        eng.upload_table(NB.line_nodes(n + 1))
        assert eng.linkest_enabled() == 0 and _code(rsa, lambda: eng.linkest_read()) == STATE
    finally:
        for b in bufs:
            b.free()
        eng.close()


_GRAPH_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import radio_sim_amd as rsa
import nbtable_ref as NB
eng = rsa.Engine(0)
eng.upload_table(NB.line_nodes(8))
for call in (lambda: eng.linkest_enable(2), lambda: eng.linkest_fold()):
    try:
        call()
    except rsa.RadioMediumError as e:
        assert e.code == -5, e
        print("REFUSED", "RM_GRAPH" in str(e))
    else:
        print("ACCEPTED")
print(int(eng.linkest_enabled()))
eng.close()
"""


def test_refused_under_graph_replay_and_without_nodes(rsa):
    """a context made under RM_GRAPH=1 -- in a fresh child process -- takes none of the extensions: enable is refused and names the
    knob; and a context without nodes refuses enable"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % (root, root)], cwd=root, env=dict(os.environ, RM_GRAPH="1"), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.split() == ["REFUSED", "True", "REFUSED", "False", "0"], p.stdout
    eng = rsa.Engine(0)
    try:
        assert _code(rsa, lambda: eng.linkest_enable(2)) == STATE and eng.linkest_enabled() == 0
        eng.upload_table(NB.line_nodes(3))
        eng.linkest_enable(2)
        assert eng.linkest_read()[0].shape == (3, 2)
    finally:
        eng.close()
