"""The scenes of tests/dense_edge_ref.py reach the branches of the dense tick they were built for -- shown from oracle values alone
(no GPU, no engine code): a scene that drifts away from its branch fails here, not silently in tests/test_gpu_dense_edges.py."""
import numpy as np
import pytest

import dense_edge_ref as D


def _candidates(sc, tk):
    """bool [slot][node]: the links the media look at -- radio on, the frame's channel, not the source itself"""
    nd = sc.nd
    src = tk.src
    ok = (nd.enabled != 0)[None, :] & (nd.channel[None, :] == nd.channel[np.maximum(src, 0)][:, None]) & (np.arange(nd.n)[None, :] != src[:, None])
    return ok & (src >= 0)[:, None]


def _int_d2(nd, src):
    """integer squared distances [source][node] of a table on an integer lattice"""
    p = np.stack([nd.x, nd.y, nd.z], axis=1)
    q = p.astype(np.int64)
    assert (q == p).all()
    d = q[src][:, None, :] - q[None, :, :]
    return (d * d).sum(axis=2), d[:, :, 2] != 0


def test_every_tick_is_small_and_needs_no_draw(O):
    """every scene through O.tick_mt once (it refuses a tick that consumes a java.util.Random draw); <= 5000 nodes"""
    names = [n for f in D.FAMILIES.values() for n in f] + ["n2n01"] + ["cells/small/%d" % k for k in range(4)]
    names += ["culled/%s/%d" % (m, k) for m in D.CULLED for k in range(2)]
    for name in names:
        sc = D.scene(O, name)
        assert sc.nd.n <= 5000, name
        for k in range(len(sc.ticks)):
            exp = D.expected(O, name, k)
            assert exp.pkt_offset[-1] == exp.count and len(exp.pkt_interference) == len(sc.ticks[k]), name


def test_lattice3d_pairs_on_the_edge_are_heard_by_udgm_alone_and_most_leave_the_plane(O):
    nd, src = D.lattice_table(O)
    assert nd.n == 2048 and D.LATTICE == (16, 16, 8) and 140 <= len(np.unique(src)) <= 160
    assert (nd.enabled == 0).sum() == 2048 // 50 and set(np.unique(nd.channel)) == {26, 58} and (26 & 31) == (58 & 31)
    # the lattice itself: ordered pairs exactly on the edge, and those with dz != 0; the disc's share of all ordered pairs
    d2, off_plane = _int_d2(nd, np.arange(nd.n))
    pairs = nd.n * (nd.n - 1)
    assert (int((d2 == 49).sum()), int(((d2 == 49) & off_plane).sum())) == (34624, 30016)
    assert (int((d2 == 81).sum()), int(((d2 == 81) & off_plane).sum())) == (38240, 34656)
    assert round(((d2 <= 49).sum() - nd.n) / pairs, 2) == 0.32 and round(((d2 <= 81).sum() - nd.n) / pairs, 2) == 0.52
    for r in (7, 9):
        sc_u, sc_c = D.scene(O, "lattice3d/udgm%d" % r), D.scene(O, "lattice3d/const%d" % r)
        tk = sc_u.ticks[0]
        d2, off_plane = _int_d2(nd, tk.src)
        cand = _candidates(sc_u, tk)
        edge = cand & (d2 == r * r)
        n_edge = int(edge.sum())
        assert n_edge > 1000 and int((edge & off_plane).sum()) * 3 >= n_edge, (r, n_edge)
        hu = D.expected(O, sc_u.name).heard(len(tk), 0, nd.n)
        hc = D.expected(O, sc_c.name).heard(len(tk), 0, nd.n)
        assert int((hu & edge).sum()) == n_edge and int((hc & edge).sum()) == 0, r      # d == range: in for UDGM, out for constant loss
        assert np.array_equal(hu, cand & (d2 <= r * r)) and np.array_equal(hc, cand & (d2 < r * r))
        # channels 26 and 58 never mix, and radios that are off hear nothing
        exp = D.expected(O, sc_u.name)
        assert (nd.channel[tk.src[exp.pkt]] == nd.channel[exp.dst]).all() and (nd.enabled[exp.dst] != 0).all()
        assert not exp.pkt_interference.any() and (exp.verdict == O.DELIVERED).all()


def _band_class(O, nd, node):
    """fast-out, fast-in or slow: the sum of squares against range^2 * (1 +- 1e-9), as dense_eval's comment states the band"""
    s = D.distance(O, (nd.x[0], nd.y[0], nd.z[0]), (nd.x[node], nd.y[node], nd.z[node])) ** 2
    r2 = D.BAND_RANGE * D.BAND_RANGE
    # (d * d instead of the sum under the root: 2 ulp apart, the classes' nearest probes are 1e-10 from the band's ends)
    return "out" if s > r2 * (1.0 + 1e-9) else "in" if s < r2 * (1.0 - 1e-9) else "slow"


@pytest.mark.parametrize("origin", list(D.BAND_ORIGINS))
def test_band_probes_take_the_fast_exits_and_the_slow_path_on_both_sides(O, origin):
    nd, probes = D.band_table(O, origin)
    assert nd.n == D.BAND_N == 1100 and len(probes) == len(D.BAND_DIRS) * len(D.BAND_E)
    assert min(p[0] for p in probes) < 1024 < max(p[0] for p in probes)                 # in both chunks
    seen = set()
    for node, u, e, d in probes:
        cls = _band_class(O, nd, node)
        assert cls == ("slow" if abs(e) <= 4e-10 else "out" if e > 0 else "in"), (origin, u, e, d)
        assert np.sign(d - D.BAND_RANGE) == np.sign(e) and abs(d / D.BAND_RANGE - 1.0 - e) < 1e-11, (origin, u, e, d)
        seen.add((cls, int(np.sign(e))))
    assert seen == {("slow", 0), ("slow", 1), ("slow", -1), ("out", 1), ("in", -1)}
    # on an axis from the near origin the probes named 0 and +-1 ulp are exactly that
    if origin == "near":
        for node, u, e, d in probes:
            if abs(e) <= D.ULP:
                assert d == (D.BAND_RANGE if e == 0 else np.nextafter(D.BAND_RANGE, np.inf if e > 0 else -np.inf)), (u, e, d)
    heard = {}
    for which in D.BAND_MODELS:
        sc = D.scene(O, "band/%s/%s" % (origin, which))
        exp = D.expected(O, sc.name)
        assert list(sc.ticks[0].src) == list(D.BAND_SOURCES)
        heard[which] = set(exp.dst[exp.pkt == 0].tolist())
    twins = {1, 1030}
    for node, u, e, d in probes:
        assert (node in heard["udgm50"]) == (e <= 0), (origin, u, e)                    # ratio > 1.0 is out: d == range is in
        assert (node in heard["const50"]) == (e < 0), (origin, u, e)                    # strict d < range
    assert heard["udgm-50"] == heard["udgm50"] and twins <= heard["udgm50"] and twins <= heard["const50"]
    assert heard["udgm50"] - twins == {p[0] for p in probes if p[2] <= 0} and heard["const50"] - twins == {p[0] for p in probes if p[2] < 0}
    assert not heard["udgm0"] and not heard["const0"]                                   # not even the co-located receivers


def test_sum9_the_sum_of_squares_and_the_distance_disagree_about_the_side(O):
    nd, probes = D.sum9_table(O)
    assert sorted(side for _, side in probes) == [-1] * 3 + [0] * 3 + [1] * 3 and min(p[0] for p in probes) < 1024 < max(p[0] for p in probes)
    for node, side in probes:
        p = (nd.x[node], nd.y[node], nd.z[node])
        s = D.sum_of_squares(p, (0, 0, 0))
        assert np.sign(s - 81.0) == side and abs(s - 81.0) <= np.spacing(81.0) and D.distance(O, (0, 0, 0), p) == 9.0
        assert (side == 0) == (p[0] == int(p[0]))
    hu, hc = (D.expected(O, "sum9/" + w) for w in ("udgm9", "const9"))
    assert set(hu.dst[hu.pkt == 0].tolist()) == {p[0] for p in probes}         # d == range, whatever the sum says
    assert not (hc.pkt == 0).any()                                             # ... and never d < range, though the sum is below 81 for three


def test_probs_every_value_occurs_on_a_link_in_range_and_only_udgm_flags(O):
    nd, src = D.lattice_table(O, probs=True)
    sc = {w: D.scene(O, "probs/" + w) for w in D.PROB_MODELS}
    tk = sc["udgm"].ticks[0]
    d2, _ = _int_d2(nd, tk.src)
    inside = _candidates(sc["udgm"], tk) & (d2 <= 49)
    bits = lambda v: np.float64(v).view(np.uint64)
    for v in D.PROB_RX:                                         # (-0.0 and 0.0 are told apart by their bits)
        assert inside[:, nd.rxprob.view(np.uint64) == bits(v)].any(), v
    for v in D.PROB_TX:
        assert inside[nd.txprob[tk.src] == v].any(), v
    exp = {w: D.expected(O, s.name) for w, s in sc.items()}
    failed = nd.txprob[tk.src] <= 0.0
    assert 0 < failed.sum() < len(tk)
    # UDGM: a frame whose transmission failed is heard all the same, every link of it interfered, and flagged
    u = exp["udgm"]
    assert np.array_equal(u.pkt_interference != 0, failed)
    assert np.array_equal(u.verdict == O.INTERFERED, failed[u.pkt]) and (u.verdict[~failed[u.pkt]] == O.DELIVERED).all()
    assert np.array_equal(u.heard(len(tk), 0, nd.n), inside & (nd.rxprob > 0.0)[None, :])
    assert failed[u.pkt].any() and (~failed[u.pkt]).any()
    # the other two read neither probability
    for w in ("const", "null"):
        assert not exp[w].pkt_interference.any() and (exp[w].verdict == O.DELIVERED).all(), w
    assert np.array_equal(exp["const"].heard(len(tk), 0, nd.n), _candidates(sc["const"], tk) & (d2 < 49))
    assert np.array_equal(exp["null"].heard(len(tk), 0, nd.n), _candidates(sc["null"], tk))


def test_shapes_cover_every_node_and_frame_count_twice(O):
    ns, ts = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049), (1, 7, 8, 9, 17)
    for n in ns:
        assert len({t for m, t in D.SHAPES if m == n}) == (1 if n == 1 else 2), n
    for t in ts:
        assert len({n for n, u in D.SHAPES if u == t and n >= t}) >= 2, t
    for model in D.SHAPE_MODELS:
        for n, t in D.SHAPES:
            sc = D.scene(O, "shapes/%s/%d/%d" % (model, n, t))
            assert sc.nd.n == n and len(sc.ticks[0]) == min(t, n) and sc.part == (0, n) and sc.force
            exp = D.expected(O, sc.name)
            # the range covers the field: the unit disc hears what the Null medium hears
            assert np.array_equal(exp.heard(min(t, n), 0, n), _candidates(sc, sc.ticks[0])), sc.name
            assert exp.count > 0 or n <= 2


def test_parts_begin_and_end_inside_waves_and_the_padding_is_where_it_should_be(O):
    assert D.PARTS == ((0, 1), (1, 1), (63, 2), (1000, 48), (1023, 1026), (5, 2044))
    nd = D.shape_table(O, 2049)
    first, count = D.PART_OFF
    assert not nd.enabled[first:first + count].any() and first % 64 and (first + count) % 64
    for model in D.SHAPE_MODELS:
        whole = D.expected(O, "shapes/%s/2049/17" % model)
        for what in D.PART_NAMES:
            sc = D.scene(O, "parts/%s/%s" % (model, what))
            exp, tk = D.expected(O, sc.name), sc.ticks[0]
            assert ((exp.dst >= sc.part[0]) & (exp.dst < sc.part[0] + sc.part[1])).all()
            if what == "off":
                assert exp.count == 0 and sc.part == D.PART_OFF
            if what == "outside":
                assert not ((tk.src >= sc.part[0]) & (tk.src < sc.part[0] + sc.part[1])).any() and exp.count > 0
            if what == "padding-only":
                assert (tk.src == -1).all() and len(tk) == 9 and exp.count == 0 and not exp.pkt_offset.any()
            if what in ("padding", "padding-part"):
                pad = tk.src < 0
                assert 0 < pad.sum() < len(tk) and exp.count > 0
                assert (np.diff(exp.pkt_offset.astype(np.int64))[pad] == 0).all()
        # a partition's links are the whole table's links at its receivers (same sources: the six index ranges)
        for p in D.PARTS:
            exp = D.expected(O, "parts/%s/%d-%d" % (model, p[0], p[1]))
            keep = (whole.dst >= p[0]) & (whole.dst < p[0] + p[1])
            assert np.array_equal(exp.pkt, whole.pkt[keep]) and np.array_equal(exp.dst, whole.dst[keep])


def test_cells_lie_on_both_sides_of_the_fused_limit_and_on_it(O):
    got = {}
    for which, (n, t) in D.CELLS.items():
        sc = D.scene(O, "cells/" + which)
        assert sc.nd.n == n and len(sc.ticks[0]) == t and sc.force and np.ptp(sc.nd.z) > 0
        got[which] = t * -(-n // 1024)
        assert D.expected(O, sc.name).count > 50_000
    assert got == {"8190": 8190, "8192": 8192, "8195": 8195}


def test_n2n01_has_ids_outside_the_matrix_and_probabilities_of_zero(O):
    sc, exp = D.scene(O, "n2n01"), D.expected(O, "n2n01")
    nd, tk, m = sc.nd, sc.ticks[0], sc.matrix.shape[0]
    assert nd.n == 300 and set(np.unique(sc.matrix)) == {0.0, 1.0} and set(np.unique(nd.rxprob)) == set(np.unique(nd.txprob)) == {0.0, 1.0}
    out = np.flatnonzero((nd.int_id <= 0) | (nd.int_id > m))
    assert len(out) == 2 and np.isin(out, tk.src).all()
    assert not np.isin(exp.dst, out).any() and not np.isin(tk.src[exp.pkt], out).any() and exp.count > 1000
    failed = nd.txprob[tk.src] <= 0.0
    assert np.array_equal(exp.pkt_interference != 0, failed) and failed.any() and not failed.all()
    assert (nd.rxprob[exp.dst] == 1.0).all() and {O.INTERFERED, O.DELIVERED} == set(exp.verdict.tolist())
