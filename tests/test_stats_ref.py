"""CPU tier of the per-node traffic counters: the REFERENCE (tests/stats_ref.py over the oracle) is held
to the conditions that make the scenes of tests/test_gpu_stats.py worth running.  If a scene misses one, the scene changes, not
the condition."""
import numpy as np
import pytest

import csma_ref as SR
import errmodel_ref as R
import stats_ref as S


def _batch(overlap, seed=None):
    """errmodel_ref.scene_batch through Replay: -> nd, lists, [TickResult], table (seed None: the verdicts before E10)"""
    nd, lists, starts, air = R.scene_batch(overlap)
    rep = R.Replay(nd, seed=R.SEED if seed is None else seed)
    res = [rep.tick(s, l, s, air)[0] for l, s in zip(lists, starts)]
    t = S.Table(nd.n)
    for l, s, w in zip(lists, starts, res):
        new = nd.packets(np.where(l >= 0, l, 0), s, air)
        new["src"] = l
        t.add_result(new, w, verdict=w.plain if seed is None else None)
    return nd, lists, res, t


@pytest.fixture(scope="module", params=[False, True], ids=["self-contained", "overlap"])
def batch(request, O):
    return _batch(request.param)


def test_sinr_batch_scene_conditions(batch):
    nd, lists, res, t = batch
    T = t.t
    for c in S.COLS:
        if c != "tx_failed":   # (the SINR medium draws no Tx failure here: the stochastic UDGM scene has that column)
            assert T[c].any(), c
    assert ((T["rx_heard"] > T["rx_delivered"]) & (T["rx_delivered"] > 0)).any()
    assert ((T["tx_frames"] > 0) & (T["rx_heard"] > 0)).any()          # a node that transmits and receives
    runs = np.concatenate([S.run_lengths(w.pkt) for w in res])
    assert ((runs > 64) & (runs % 64 != 0)).any()                       # a run that crosses a wave boundary
    assert (T["tx_frames"] >= 2).any()                                  # a node that transmits in two ticks of the batch
    assert max(np.bincount(w.dst, minlength=nd.n).max() for w in res if w.count) >= 8   # contention on one record
    assert max(w.count for w in res) > 16384                            # more than one grid stride
    assert any(w.count % 64 for w in res)
    assert any(len(l) == 0 for l in lists) and any((l < 0).any() for l in lists)       # an empty tick, padding entries
    assert t.counted == sum(1 for l in lists if len(l)) and t.skipped == 0
    # the sums are what the columns mean
    assert T["tx_links_heard"].sum() == T["rx_heard"].sum() == sum(w.count for w in res)
    assert T["tx_links_delivered"].sum() == T["rx_delivered"].sum()
    assert T["tx_frames"].sum() == sum(int((l >= 0).sum()) for l in lists)


def test_error_model_changes_the_delivered_columns(O):
    _, _, _, plain = _batch(True)
    _, _, _, e10 = _batch(True, seed=R.SEED)
    for c in S.COLS:
        if c not in ("rx_delivered", "tx_links_delivered"):
            np.testing.assert_array_equal(plain.t[c], e10.t[c], err_msg=c)
    assert int(plain.t["rx_delivered"].sum()) - int(e10.t["rx_delivered"].sum()) >= 50
    assert int(plain.t["tx_links_delivered"].sum()) - int(e10.t["tx_links_delivered"].sum()) >= 50


def test_lone_and_serial_scenes(O):
    nd, srcs, start, air = R.scene_lone()
    w, _ = R.Replay(nd).tick(0, srcs, start, air)
    t = S.Table(nd.n)
    t.add_result(nd.packets(srcs, start, air), w)     # (with E10's verdicts: what the GPU test of the lone forms counts)
    assert ((t.t["rx_heard"] > t.t["rx_delivered"]) & (t.t["rx_delivered"] > 0)).any()
    assert t.t["tx_frames"].sum() == len(srcs) and t.t["rx_air_us"].sum() == air * w.count
    nd, srcs, starts, _, air = R.scene_serial()
    rep, t = R.Replay(nd), S.Table(nd.n)
    for q, s in zip(srcs, starts):
        w, _ = rep.tick(int(s), [q], int(s), air)
        t.add_result(nd.packets([q], int(s), air), w, verdict=w.plain)
    assert t.counted == len(srcs) and t.t["tx_links_heard"].sum() > 100


def test_stochastic_udgm_scene_conditions(O):
    sc = S.scene_udgm()
    nd, kind, params, pk, _, _ = sc
    res = S.oracle_tick(sc)
    T = S.table_of(sc, res).t
    for c in S.COLS:
        assert T[c].any(), c
    assert res.pkt_draws.sum() > 100 and T["tx_failed"].sum() == res.pkt_interference.sum() > 0
    # links lost to the rxProbability draw: delivered without any draw, not delivered here, and their frame's Tx draw went well
    sure = S.oracle_tick((nd, kind, {}, pk, None, None))
    np.testing.assert_array_equal(sure.pkt, res.pkt)
    np.testing.assert_array_equal(sure.dst, res.dst)
    lost = (sure.verdict == O.DELIVERED) & (res.verdict != O.DELIVERED) & (res.pkt_interference[res.pkt] == 0)
    assert lost.sum() >= 20
    # about three links per frame: a wave of the pass holds the links of many frames
    assert S.most_packets_in_a_wave(res.pkt) >= 3 and res.count > 64


def test_other_media_scenes(O):
    for scene, least in ((S.scene_udgm_const(), 1000), (S.scene_n2n(), 100), (S.scene_null(), 6 * 2999)):
        res = S.oracle_tick(scene)
        assert res.count >= least
        t = S.table_of(scene, res)
        assert t.t["rx_heard"].sum() == res.count and t.counted == 1
    assert S.oracle_tick(S.scene_n2n()).pkt_draws.sum() > 0


def test_csma_scene_conditions(O):
    """csma_ref's `multi`: deferred candidates and slots never made add nothing; the frames counted are the RM_CSMA_SENT packets"""
    n_ticks, _ = SR.SCENES["multi"]
    r = SR.run(O, "multi")
    assert len(r.exp) == n_ticks
    t = S.Table(6000)   # (cca_ref.Scene "multi")
    for b in range(n_ticks):
        t.add_expected(r.exp[b], int(r.n_exp[b]))
    assert t.t["tx_frames"].sum() == int((r.status == SR.SENT).sum()) > 0
    assert sum(int((k < 0).sum()) for k in r.kept) > 0            # deferred candidates and slots never made
    assert sum(int((m < 0).sum()) for m in r.made) > 0            # ... of which some were never made
    assert t.counted == n_ticks


def test_table_arithmetic():
    """the accumulator on a hand-made tick: three frames (one padding), four links"""
    t = S.Table(5)
    t.add(src=[2, -1, 4], air_us=[100, 100, 300], failed=[0, 0, 1], pkt=[0, 0, 2, 2], dst=[1, 3, 1, 2],
          verdict=[O_DELIVERED, 1, O_DELIVERED, 1])
    want = np.zeros(5, dtype=S.DTYPE)
    want[2] = (1, 0, 100, 2, 1, 1, 0, 300)
    want[4] = (1, 1, 300, 2, 1, 0, 0, 0)
    want[1] = (0, 0, 0, 0, 0, 2, 2, 400)
    want[3] = (0, 0, 0, 0, 0, 1, 0, 100)
    np.testing.assert_array_equal(t.t, want)
    t.add([], [], [], [], [], [])
    assert t.totals() == {"ticks_counted": 1, "ticks_skipped": 0}


O_DELIVERED = 2
