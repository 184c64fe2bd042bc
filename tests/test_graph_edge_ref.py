"""The scenes of tests/graph_edge_ref.py reach the parts of the graph queries' walk they were built for -- shown from the reference
alone (the oracle's links, hops_ref.tree, routes_ref.tree; no GPU, no engine code): a scene that drifts away from its edge fails
here, not silently in tests/test_gpu_graph_edges.py."""
import numpy as np
import pytest

import graph_edge_ref as G
import hops_ref as H
import neighbors_ref as N
import routes_ref as R

WIDE_CAP = dict(G.Q["OQPSK"], max_link_cost=65535)


def _bits(r):
    return int(N.bits([r])[0])


# ---- 1. lattice3d ------------------------------------------------------------------------------------------------------------------

def test_lattice3d_ties_in_shells_and_ends_on_the_level(O):
    """LEVEL: an interior node has 122 links in tie groups of 6, 12, 8, 6, 24, 24, 12, 30, the last 30 at exactly the sensitivity
    (measured; the same in both directions).  K = 1, 2, 4 cut the first group, K = 8 and 16 the second: at all 27 interior nodes
    the K-th and the (K + 1)-th entry tie for every K of N.KS."""
    nd, params, found = G.lattice3d("LEVEL")
    _, at = G.lattice3d_table()
    assert nd.n == 729 and len(np.unique(nd.z)) == 9 and (at != np.arange(nd.n)).sum() > 700
    sens = params["ld_sensitivity_dbm"]
    assert _bits(sens) == _bits(G.pair_rssi(90.0)) and -99.0 < sens < -98.0
    inner = G.interior()
    assert len(inner) == 27
    for d in G.DIRS:
        for j in inner:
            sh = G.shells(found[d], j)
            assert len(found[d][j]) >= 100 and [c for _, c in sh] == [6, 12, 8, 6, 24, 24, 12, 30]
            assert sh[-1][1] >= 20 and _bits(sh[-1][0]) == _bits(sens)                    # the last shell is AT the level
            assert not any(abs(r - sens) < 1e-6 for r, _ in found[d][j] if _bits(r) != _bits(sens))   # and nothing else is near it
        for K in N.KS:
            tied = [j for j in inner if N.rank(found[d][j], K + 1)[1][K - 1] == N.rank(found[d][j], K + 1)[1][K]]
            assert tied, (d, K)
        # the tie-break is by node index, and the permutation made it disagree with the order of the lattice's points
        peer = N.rank(found[d][inner[0]], 6)[0]
        assert peer == sorted(peer) and sorted(np.argsort(at)[peer].tolist()) != np.argsort(at)[peer].tolist()


def test_lattice3d_hop_thresholds_are_shells(O):
    """LEVEL, corner root: at min_rssi_dbm equal to a shell's own rssi the shell stays, at the next double it goes -- the two
    reference trees differ for every one of the eight shells; all thresholds are at or above the sensitivity.  688 nodes have more
    than one parent candidate, 198 of them a tied first pair (measured)."""
    nd, params, found = G.lattice3d("LEVEL")
    for d in G.DIRS:
        sh = G.shells(found[d], G.interior()[0])
        assert len(sh) == 8
        for r, _ in sh:
            assert r >= params["ld_sensitivity_dbm"]
            a, b = G.hop_tree("LEVEL", d, "corner", r), G.hop_tree("LEVEL", d, "corner", G.up(r))
            assert (a["hop"] != b["hop"]).any() and a["totals"]["reached"] >= b["totals"]["reached"] >= 1
        w = G.hop_tree("LEVEL", d, "corner")
        cand = H.candidates(nd.n, found[d], w)
        assert w["totals"] == {"reached": 729, "max_hop": 5, "roots": 1}
        assert sum(1 for c in cand.values() if len(c) > 1) >= 500
        assert sum(1 for c in cand.values() if len(c) > 1 and c[0][0] == c[1][0]) >= 150


def test_lattice3d_route_costs_and_ties(O):
    """MARGINAL, OQPSK, us_per_bit 4, air_us 4064: the shells cost 128 (seven shells), 129, 132, 147, 204, 431, 1787, and two
    shells do not count.  Corner root (measured): 729 reached, max_cost 644, 660 nodes with more than one parent candidate, 213 of
    them with the first two tied in rssi, 370 nodes deeper than their hop count.  A cap of 128 and one of 129 give different
    routes."""
    nd, params, found = G.lattice3d("MARGINAL")
    for d in G.DIRS:
        costs = [R.link_cost(WIDE_CAP, r) for r, _ in G.shells(found[d], G.interior()[0])]
        assert costs == [128] * 7 + [129, 132, 147, 204, 431, 1787, None, None]
        w = G.route_tree("MARGINAL", d, "corner", "OQPSK")
        assert w["totals"] == {"reached": 729, "roots": 1, "max_cost": 644}
        cand = R.candidates(nd.n, found[d], w, G.Q["OQPSK"])
        assert sum(1 for c in cand.values() if len(c) > 1) >= 500
        assert sum(1 for c in cand.values() if len(c) > 1 and c[0][0] == c[1][0]) >= 150
        assert (R.depth(w) > G.hop_tree("MARGINAL", d, "corner")["hop"]).sum() >= 250
        a, b = (G.route_tree("MARGINAL", d, "corner", "OQPSK", max_link_cost=c) for c in (128, 129))
        assert (a["cost"] != b["cost"]).any() and a["totals"]["max_cost"] == 768 and b["totals"]["max_cost"] == 644
        sh = G.shells(found[d], G.interior()[0])
        for k in G.ROUTE_SHELLS:                                      # the last 128 shell, the 129 shell and the 204 shell
            r = sh[k][0]
            assert r > params["ld_sensitivity_dbm"]
            a, b = (G.route_tree("MARGINAL", d, "corner", "OQPSK", min_rssi_dbm=m) for m in (r, G.up(r)))
            assert (a["cost"] != b["cost"]).any() or (a["parent"] != b["parent"]).any(), k


# ---- 2. wide -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(G.WIDE_L))
def test_wide_probes_straddle_the_level_at_the_slacks_edge(O, path):
    """64 in-probes and 64 out-probes, each pair one double of t apart: every in-probe is a link of the source and no out-probe is,
    in both directions; all lie within 1e-9 dB of the level (measured: within 1.3e-11).  The fp32 frame is as coarse as the boxes
    path trusts: spacing above 0.005 m at the cluster, slack 0.0475 m (boxes) and 0.0537 m (scan, beyond the limit of 0.05)."""
    nd, params, found, who = G.wide(path)
    lv = params["ld_sensitivity_dbm"]
    assert _bits(lv) == _bits(G.pair_rssi(30.0)) and nd.n == 729 + 1 + 128
    for d in G.DIRS:
        got = {far: r for r, far in found[d][who["src"]]}
        assert all(k in got for k in who["in"]) and not any(k in got for k in who["out"])
        assert all(0.0 <= got[k] - lv < 1e-9 for k in who["in"])
        assert len(got) == 64
    # the out-probes' rssi, by the oracle with the sensitivity out of the way
    low = N.links(nd, dict(params, ld_sensitivity_dbm=lv - 1.0), N.HEARD_BY, [who["src"]])[who["src"]]
    out = {far: r for r, far in low if far in set(who["out"])}
    assert len(out) == 64 and all(0.0 < lv - r < 1e-9 for r in out.values())
    bound, slack = G.frame(nd)
    L = G.WIDE_L[path]
    assert float(np.spacing(np.float32(L - bound))) > 0.005 and abs(bound - L / 2) < 100.0
    assert (0.04 < slack <= 0.05) if path == "boxes" else (0.05 < slack < 0.06)
    assert H.tree(nd.n, found[N.HEARD_BY], [who["src"]])["totals"] == {"reached": 129, "max_hop": 2, "roots": 1}


# ---- 3. specials -------------------------------------------------------------------------------------------------------------------

def test_specials_table_and_the_oracles_answers(O):
    """four channels on one mask bit (one negative), 70 radios off over all four, powers NaN / +inf / -inf / 1e300, receive
    probabilities NaN / -0.0 / -1.0 / 5e-324.  The oracle: +inf and 1e300 are heard by every enabled same-channel listener, NaN and
    -inf by nobody, and all four hear normally; NaN and the denormal listen, -0.0 and -1.0 do not (but are heard).  Measured: 2675
    HEARS links whose transmitter is off."""
    nd, params, who = G.specials()
    found = G.specials_links()
    c = sorted(set(nd.channel.tolist()))
    assert len(c) == 4 and c[0] < 0 and len({v & 31 for v in c}) == 1
    off = set(who["off"])
    assert len(off) == 70 > 64 and {int(nd.channel[j]) for j in off} == set(c)
    assert [_bits(v) for v in nd.txpower[who["power"]]] == [_bits(v) for v in G.ODD_POWER]
    assert [_bits(v) for v in nd.rxprob[who["rxprob"]]] == [_bits(v) for v in G.ODD_RXPROB]
    listens = (nd.enabled != 0) & ~(nd.rxprob <= 0.0)
    deg = {d: {j: len([1 for r, _ in found[d][j] if r == r]) for j in who["power"] + who["rxprob"]} for d in G.DIRS}
    p_nan, p_inf, p_ninf, p_big = who["power"]
    for j in (p_inf, p_big):
        assert deg[N.HEARD_BY][j] == int((listens & (nd.channel == nd.channel[j])).sum()) - 1 > 150
    for j in (p_nan, p_ninf):
        assert deg[N.HEARD_BY][j] == 0
    assert all(deg[N.HEARS][j] > 50 for j in who["power"])
    r_nan, r_nzero, r_neg, r_den = who["rxprob"]
    assert deg[N.HEARS][r_nan] > 50 and deg[N.HEARS][r_den] > 50 and deg[N.HEARS][r_nzero] == 0 and deg[N.HEARS][r_neg] == 0
    assert all(deg[N.HEARD_BY][j] > 50 for j in who["rxprob"])
    # a radio that is off transmits: it is a HEARS link of same-channel nodes ...
    assert sum(1 for j in range(nd.n) for _, p in found[N.HEARS][j] if p in off) >= 1000
    # ... and only the exact channel compare keeps the off radios of the three aliasing channels out: with every channel made one,
    # the same table has off-radio HEARS links that it does not have as it is
    one = N._copy(nd)
    one.channel[:] = c[1]
    merged = N.links(one, params, N.HEARS)
    extra = sum(1 for j in range(nd.n) if listens[j] for r, p in merged[j]
                if p in off and nd.channel[p] != nd.channel[j] and p not in {f for _, f in found[N.HEARS][j]})
    assert extra >= 1000
    # the +inf node as a root reaches every same-channel listener in one hop
    w = H.tree(nd.n, found[N.HEARS], [p_inf])
    assert (w["hop"] == 1).sum() == deg[N.HEARD_BY][p_inf]


def test_specials_after_the_updates(O):
    """the four odd powers back to 0 dBm: the largest power of the table falls from +inf to 0 and every row that held the loud
    nodes shrinks; every power NaN: no link at all"""
    nd0, params, who = G.specials()
    found = G.specials_links()
    nd = N._copy(nd0)
    nd.txpower[who["power"]] = 0.0
    calm = N.links(nd, params, N.HEARS)
    for j in who["power"][1::2]:                                          # (+inf and 1e300)
        hears = lambda ls: sum(1 for v in ls.values() for _, p in v if p == j)
        assert hears(calm) < 100 and hears(found[N.HEARS]) > 150
    for j in who["power"][0::2]:                                          # (NaN and -inf: heard by nobody before)
        assert sum(1 for v in calm.values() for _, p in v if p == j) > 50
    nd.txpower[:] = float("nan")
    for d in G.DIRS:
        assert sum(len([1 for r, _ in v if r == r]) for v in N.links(nd, params, d).values()) == 0


# ---- 4. sizes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", G.SIZES)
def test_sizes(O, n):
    """65, 1023, 1024 and 1025 nodes of a 16 x 8 x 8 lattice under MARGINAL: one group of 64 and one node, a box of 1024 less one,
    full, and one more.  Every node is reached from node 0 in four hops, and routes run deeper than hops."""
    nd, params, found, at = G.sizes(n)
    assert nd.n == n and (n <= 65 or len(np.unique(nd.z)) >= 8)
    for d in G.DIRS:
        h = H.tree(n, found[d], [0])
        r = R.tree(n, found[d], [0], G.Q["OQPSK"])
        assert h["totals"] == {"reached": n, "max_hop": 4, "roots": 1} and r["totals"]["reached"] == n
        assert (R.depth(r) > h["hop"]).sum() >= n // 4
        assert max(len(v) for v in found[d].values()) > 16


# ---- 5. many_roots -----------------------------------------------------------------------------------------------------------------

def test_many_roots_lists(O):
    """the lists are longer than one stride of the seeding kernels (16 384 entries), and each of the long ones holds a root that
    occurs only behind the first stride (in "40000": one in the second stride, one in the third)"""
    lists, late = G.root_lists()
    n = G.lattice3d_table()[0].n
    assert G.STRIDE == 16384 and {k: len(v) for k, v in lists.items()} == {"16384": 16384, "16385": 16385, "40000": 40000, "every": 23 * n, "outside": 16389}
    assert len(set(lists["16384"].tolist())) == 97 and not set(late) & set(lists["16384"].tolist())
    assert np.flatnonzero(lists["16385"] == late[0]).tolist() == [16384]
    c = lists["40000"]
    assert np.flatnonzero(c == late[1]).tolist() == [G.STRIDE + 5] and np.flatnonzero(c == late[2]).tolist() == [39999] and 39999 >= 2 * G.STRIDE
    assert len(set(c.tolist())) == 99
    e = lists["every"]
    assert len(e) > G.STRIDE and set(e.tolist()) == set(range(n)) and e[:G.STRIDE].max() < n - 1
    o = lists["outside"]
    assert o[G.STRIDE:].tolist() == [-1, n, late[0], 2 ** 31 - 1, -1]
    nd, _, found = G.lattice3d("MARGINAL")
    for d in G.DIRS:
        for label, roots, k in (("16384", lists["16384"], 97), ("16385", lists["16385"], 98), ("40000", c, 99), ("every", e, n), ("outside", o, 98)):
            assert H.tree(n, found[d], roots)["totals"]["roots"] == k
        # the late roots matter: without them the tree is another one
        assert (H.tree(n, found[d], lists["16385"])["hop"] != H.tree(n, found[d], lists["16384"])["hop"]).any()


# ---- 6. hub ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", G.HUB_M)
def test_hub(O, m):
    """K = 16 against a degree of 15, 16 and 17: the last place is empty, filled by the last link, or contested inside the second
    tie group (the 17th link ties with the 16th and loses on its node index)"""
    nd, params, hub = G.hub(m)
    assert nd.n == 1 + m + G.N_FILL > 64
    for d in G.DIRS:
        ls = N.links(nd, params, d)
        assert len(ls[hub]) == m and [c for _, c in G.shells(ls, hub)] == [6, m - 6]
        assert all(len(ls[j]) == 0 for j in range(nd.n) if nd.y[j] == -5000.0)
        peer, rb, deg = N.rank(ls[hub], 16)
        assert deg == m and (peer[15] == -1) == (m == 15) and peer[:6] == sorted(peer[:6]) and peer[6:m][:10] == sorted(peer[6:m][:10])
        if m == 17:
            p17, r17, _ = N.rank(ls[hub], 17)
            assert r17[15] == r17[16] and p17[15] < p17[16] and peer[15] == p17[15]


# ---- 7. bounds ---------------------------------------------------------------------------------------------------------------------

def test_bounds(O):
    """V's direct link costs exactly 385 = cost[P] + 129 and the three-hop route 384; X hangs on a link of exactly 431 and Y on one of
    exactly 1787: caps of 430 / 431 and of 1786 / 1787 decide them"""
    nd, params, found, w = G.bounds()
    assert nd.n > 64
    for d in G.DIRS:
        cost = {(a, b): R.link_cost(WIDE_CAP, r) for a in w for r, far in found[d][w[a]] for b in w if w[b] == far}
        assert cost[("R", "A")] == cost[("A", "P")] == cost[("P", "V")] == 128 and cost[("R", "V")] == G.RELAX_DIRECT == 385
        assert cost[("R", "P")] > 256 and ("A", "V") not in cost and ("V", "A") not in cost
        assert cost[("V", "X")] == 431 and cost[("X", "Y")] == 1787 and {k for k in cost if "X" in k or "Y" in k} == {("V", "X"), ("X", "V"), ("X", "Y"), ("Y", "X")}
        want = {128: (0, 128, 256, 384, None, None), 430: (0, 128, 256, 384, None, None), 431: (0, 128, 256, 384, 815, None),
                1786: (0, 128, 256, 384, 815, None), 1787: (0, 128, 256, 384, 815, 2602), 65535: (0, 128, 256, 384, 815, 2602)}
        for cap, costs in want.items():
            t = R.tree(nd.n, found[d], [w["R"]], dict(G.Q["OQPSK"], max_link_cost=cap))
            assert tuple(None if t["cost"][w[k]] == R.UNREACHED else int(t["cost"][w[k]]) for k in "RAPVXY") == costs, cap
            assert t["totals"]["reached"] == sum(1 for v in costs if v is not None)
        # V is first labelled by the root itself: the hop query reaches it in one hop
        assert H.tree(nd.n, found[d], [w["R"]])["hop"][w["V"]] == 1
