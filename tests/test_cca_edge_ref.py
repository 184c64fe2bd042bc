"""CPU tier of tests/test_gpu_cca_edges.py: every scene of tests/cca_edge_ref.py is held to the conditions that make it reach the branch
it is there for, so that the GPU test cannot pass vacuously.  The conditions are written against DESIGN.md's description of the index
(sections 4.9 - 4.11), not against engine code: the frame is the bounding box, the grid is 64 x 64 over a square whose half-width is
the largest half-extent -- so a cell's side is at least (largest extent) / 64; a cell holds 16 frames for the query and the lone gate
and 64 for the batch, the rest goes to the EVERY list, which the query stages 256 records at a time; one workgroup of 1024 threads
resolves a batch and workgroups of 1024 scan it.  Everything is computed with the oracle alone."""
import time

import numpy as np

import cca_batch_ref as BR
import cca_edge_ref as ER
import energy_ref as R

HIGH_WORD_DBM = -48.16          # 10 log10(2^-16) = -48.1648: a Q80 sum at or above 2^64


def _timed(O, name):
    t = time.time()
    r = ER.run(O, name)
    print("%s: oracle chain %.1f s" % (name, time.time() - t))
    return ER.scene(O, name), r


def _in_box(sc, frames):
    cx, cy, side = sc.box
    return (frames["x"] >= cx) & (frames["x"] <= cx + side) & (frames["y"] >= cy) & (frames["y"] <= cy + side)


def test_hotspot_meets_its_conditions(O):
    sc, r = _timed(O, "hotspot")
    nd = sc.nd
    assert sc.box[2] < ER.cell_side(nd) / 2, "the hot spot may lie in more than 4 cells"
    # (a), (b): live hot-spot frames in the window; the pigeonhole over 4 cells of 16 and a chunk of 256
    for k, t in ((ER.HOT_QUERY, sc.t_cca[ER.HOT_QUERY]), (ER.HOT_GATE, sc.t_cca[ER.HOT_GATE])):
        frames = ER.live(r.before[k], t)
        assert int(_in_box(sc, frames).sum()) >= 4 * (16 + 256) + 4
    first, last = ER.HOT_BATCH
    cand = np.concatenate(r.lists[first:last])
    in_hot = lambda nodes: (nodes >= sc.hot[0]) & (nodes <= sc.hot[-1])
    assert int(_in_box(sc, r.before[first]).sum()) + int(in_hot(cand).sum()) >= 4 * 64 + 4
    # the high word, in the query and among the candidates
    tq = sc.t_cca[ER.HOT_QUERY]
    e, f, cnt, q = ER.sense(O, sc, r.before[ER.HOT_QUERY], tq, sc.query_nodes, q80=True)
    assert (e > HIGH_WORD_DBM).any() and max(q) >> 64 and (e < -90.0).any()
    assert (r.energy[ER.HOT_GATE] > HIGH_WORD_DBM).any() and all((x[x == x] > HIGH_WORD_DBM).any() for x in r.energy[first:last])
    assert set(f.tolist()) >= {0, R.ED_BUSY, R.ED_TRANSMITTING | R.ED_BUSY}
    # a sum whose low words carry (whatever the order of the adds): one in the query, one among the lone tick's and the batch's candidates
    carries = lambda k, nodes: next((int(j) for j in nodes if j >= 0 and ER.low_words_carry(
        O, sc, ER.live(r.before[k], sc.t_cca[k]), sc.t_cca[k], int(j))), None)
    carrying = [carries(ER.HOT_QUERY, sc.query_nodes[np.array(q) >> 64 > 0][:6]), carries(ER.HOT_GATE, r.lists[ER.HOT_GATE][r.energy[ER.HOT_GATE] > HIGH_WORD_DBM][:6]),
                carries(first, r.lists[first][r.energy[first] > HIGH_WORD_DBM][:6])]
    assert None not in carrying, carrying
    # the forced channel differs from the own channels
    forced = R.channel_energy(O, sc.model(O), nd, r.before[ER.HOT_QUERY], tq, nodes=sc.query_nodes, channel=13, threshold=sc.threshold)
    assert (forced[0] != e).any()
    # the outcome mix among hot-spot candidates, the transmitting flag, the wrong readings
    for k in range(ER.HOT_GATE, last):
        hot = in_hot(r.lists[k])
        if k != first:      # (ticks >= 1 of the batch, and the lone tick)
            assert (r.flags[k][hot] == 0).any() and (r.flags[k][hot] & R.ED_BUSY).any(), k
        assert (r.flags[k][hot] & R.ED_TRANSMITTING).any(), k
    all_kept, window_only = BR.wrong_readings(O, sc, r, first, last)
    flags = np.concatenate(r.flags[first:last])
    assert (np.concatenate(all_kept) != flags).any() and (np.concatenate(window_only) != flags).any()
    print("hotspot: deferred per step", [int((x != 0).sum()) for x in r.flags[ER.HOT_GATE:last]], "carrying", carrying[:4],
          "max Q80 bits", max(q).bit_length())


def test_bigtick_meets_its_conditions(O):
    sc, r = _timed(O, "bigtick")
    assert tuple(len(s) for s in r.lists[1:]) == ER.BIG_SIZES and sum(ER.BIG_SIZES) > 2048
    assert (r.lists[1][:1024] < 0).any() and (r.lists[1][1024:] < 0).any()
    only_because, kept_although = [], []
    for long_k, short_k in ((1, 2), (3, 4)):
        high = r.lists[long_k][1024:]
        high_flags = r.flags[long_k][1024:]
        tc = sc.t_cca[short_k]
        kept_high = set(high[(high >= 0) & (high_flags == 0)].tolist())
        deferred_high = high[(high >= 0) & (high_flags != 0)]
        before = r.before[short_k]
        nd = sc.nd
        # (only to keep the search short: a frame more than 150 m away is below the threshold even with 3 sigma of shadowing)
        close = lambda j, nodes: [int(s) for s in nodes if nd.channel[s] == nd.channel[j] and np.hypot(nd.x[s] - nd.x[j], nd.y[s] - nd.y[j]) < 150.0]
        for i, j in enumerate(r.lists[short_k].tolist()):
            if r.flags[short_k][i] == R.ED_BUSY:           # deferred only because of ONE kept frame of a slot >= 1024?
                for s in close(j, sorted(kept_high)):
                    if not ER.sense(O, sc, before[before["src"] != s], tc, [j])[1][0]:
                        only_because.append((short_k, j, int(s)))
            elif r.flags[short_k][i] == 0:                 # kept, although a deferred candidate of a slot >= 1024 would have made it busy?
                for s in close(j, deferred_high):
                    frame = sc.nd.packets(np.array([s]), sc.start[long_k], sc.airs[long_k])
                    if ER.sense(O, sc, np.concatenate([before, frame]), tc, [j])[1][0] & R.ED_BUSY:
                        kept_although.append((short_k, j, int(s)))
                        break
    assert only_because and kept_although, (only_because, kept_although)
    print("bigtick: deferred only because of a kept slot >= 1024:", only_because[:3], "kept although:", kept_although[:3],
          "deferred per tick", [int((x != 0).sum()) for x in r.flags[1:]])


def test_times_meets_its_conditions(O):
    sc, r = _timed(O, "times")
    T = ER.TIMES
    assert len(set(t[3] for t in T)) == len(T) and T[4][3] == 0                                   # an air time of its own per tick, one of 0
    assert T[1][2] + T[1][3] == T[6][1] and T[3][2] + T[3][3] == T[5][1] + 1                      # exact end; one past the sample
    assert T[2][:3] == T[3][:3] and T[2][1] == T[2][2]                                            # two ticks at one instant, sample == start
    assert T[0][2] + T[0][3] == T[5][1] == T[4][1] + 1                                            # the window's frame
    for what, change, step in ER.TIMES_MOVES:
        moved = ER.Run(O, sc, change=change)
        differ = int((moved.flags[step] != r.flags[step]).sum())
        print("times: %s: %d flags of step %d flip when the boundary moves by 1 us" % (what, differ, step))
        assert differ > 0, what
        for k in range(1, step):
            np.testing.assert_array_equal(moved.flags[k], r.flags[k])
    flags = np.concatenate(r.flags[1:])
    assert (flags == 0).any() and (flags & R.ED_BUSY).any()


def test_sparse512_meets_its_conditions(O):
    sc, r = _timed(O, "sparse512")
    sizes = [len(s) for s in r.lists]
    assert len(sizes) == ER.MAX_BATCH and sizes[:3] == [0, 0, 0] and sizes[-2:] == [0, 0] and not any(sizes[8:108])
    full = [k for k in range(ER.MAX_BATCH) if sizes[k]]
    assert tuple(full) == ER.SPARSE_FULL and 3 <= min(sizes[k] for k in full) and max(sizes) <= 40
    both = [k for k in full if (r.flags[k][r.lists[k] >= 0] == 0).any() and (r.flags[k] != 0).any()]
    assert len(both) >= 3, both
    assert sc.airs[0] > 3 * (sc.t_begin[1] - sc.t_begin[0])                                      # frames overlap several ticks
    print("sparse512: ticks with both outcomes", both)


def test_flat_meets_its_conditions(O):
    sc, r = _timed(O, "flat")
    nd, mdl = sc.nd, sc.model(O)
    assert mdl.ld_exponent == 0.0
    level = nd.txpower - mdl.ld_pl0_db
    assert 0.4 <= (level > mdl.ld_ifloor_dbm + 9.0).mean() <= 0.6 and ((level > mdl.ld_ifloor_dbm + 9.0) | (level < mdl.ld_ifloor_dbm - 9.0)).all()
    assert len(r.before[ER.FLAT_QUERY]) >= 256                                                    # the grid is selected by count
    tq = sc.t_cca[ER.FLAT_QUERY]
    e, f, cnt = ER.sense(O, sc, r.before[ER.FLAT_QUERY], tq, sc.query_nodes)
    assert cnt.min() == 0 and cnt.max() >= 24 and (f & R.ED_BUSY).any() and (f == 0).any()
    first, last = ER.FLAT_BATCH
    for k in range(ER.FLAT_GATE, last):
        assert (r.flags[k] == 0).any() and (r.flags[k] & R.ED_BUSY).any() and (r.flags[k] & R.ED_TRANSMITTING).any(), k
    all_kept, window_only = BR.wrong_readings(O, sc, r, first, last)
    flags = np.concatenate(r.flags[first:last])
    print("flat: counting frames", int(cnt.min()), "..", int(cnt.max()), "deferred per step", [int((x != 0).sum()) for x in r.flags[ER.FLAT_GATE:last]],
          "differ from all-kept", int((np.concatenate(all_kept) != flags).sum()), "from window-only", int((np.concatenate(window_only) != flags).sum()))


def test_far_scene_meets_its_conditions(O):
    nd, params, srcs, frames, far = ER.far_scene(O)
    assert far not in srcs
    half = max(np.ptp(nd.x), np.ptp(nd.y)) / 2
    assert float(np.spacing(np.float32(half))) > 0.05                                              # fp32 cannot hold this frame's positions
    e, f, cnt = R.channel_energy(O, O.model(4, **params), nd, frames, 0, nodes=np.array([far, 0, 1], dtype=np.int32), threshold=-90.0)
    assert e[0] == -100.0 and cnt[0] == 0 and f[0] == 0


def test_energy_ref_q80_is_optional(O):
    nd, params, srcs, frames, _ = ER.far_scene(O)
    nodes = np.arange(40, dtype=np.int32)
    three = R.channel_energy(O, O.model(4, **params), nd, frames, 0, nodes=nodes)
    four = R.channel_energy(O, O.model(4, **params), nd, frames, 0, nodes=nodes, q80=True)
    assert len(three) == 3 and len(four) == 4 and all(isinstance(q, int) for q in four[3])
    noise = O.lib().orc_det_pow10(-10.0)
    for e, q in zip(four[0], four[3]):
        assert e == 10.0 * O.lib().orc_det_log10(R.from_fixed(q) + noise)
