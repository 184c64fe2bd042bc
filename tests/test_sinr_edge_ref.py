"""The scenes of tests/sinr_edge_ref.py reach the branches they were built for -- shown from oracle values alone (no GPU, no engine
code): a scene that drifts away from its branch fails here, not silently in tests/test_gpu_sinr_edges.py."""
import numpy as np

import sinr_edge_ref as S


def _links(res):
    return {(int(p), int(d)): k for k, (p, d) in enumerate(zip(res.pkt, res.dst))}


def test_every_scene_is_small_and_its_sums_are_inside_the_exact_range(O):
    """n <= 300, <= 20 ticks; no receiver's whole sum reaches 2^47 mW: with P = the strongest power any frame
    has at any node, frames-on-the-air * P bounds every sum"""
    for names in S.FAMILIES.values():
        for name in names:
            sc, r = S.scene(O, name), S.run(O, name)
            assert sc.nd.n <= 300 and len(sc.ticks) <= 20
            most = max([len(b) + len(n) for b, n in zip(r.before, r.new)] + [len(r.onair) + len(sc.tail)])
            mdl = sc.model(O)
            power = max([float(sc.nd.txpower.max())] + [float(n["txpower"].max()) for n in r.new if len(n)])
            top = power - mdl.ld_pl0_db + mdl.ld_sigma_db * mdl.ld_clip          # E1 / E2: the path loss beyond pl0 is >= 0, |g| <= clip
            assert most * 10.0 ** (top / 10.0) < 2.0 ** 47, name


def test_hot_carries_twice_uses_the_high_word_and_aliases_channels(O):
    sc, r = S.scene(O, "hot"), S.run(O, "hot")
    exp, frames = r.exp[0], r.new[0]
    assert (exp.count, int((exp.verdict == O.INTERFERED).sum()), int((exp.verdict == O.DELIVERED).sum())) == (781, 639, 142)
    # some heard link's receiver: the sum over the tick's frames on its channel carries out of the low word twice, high word in use
    best = (0, 0)
    for j in np.unique(exp.dst):
        carries, high = S.low_word_carries(S.q80_terms(O, sc, frames, int(j), sc.nd.channel[j]))
        if carries >= 2 and high > 0:
            best = (carries, high)
            break
    assert best[0] >= 2 and best[1] > 0
    # d < d0 on a heard link
    d = np.hypot(frames["x"][exp.pkt] - sc.nd.x[exp.dst], frames["y"][exp.pkt] - sc.nd.y[exp.dst])
    assert (d < sc.params["ld_d0"]).any() and (d > sc.params["ld_d0"]).any()
    # for each two of the three channels, in both orders: a frame on one and an enabled node on the other that the frame reaches
    # -- only the exact channel test tells them apart (all three are bit 28 of a 32-bit mask)
    assert len({c & 31 for c in S.HOT_CHANNELS}) == 1
    for a in S.HOT_CHANNELS:
        for b in S.HOT_CHANNELS:
            if a == b:
                continue
            found = False
            for k in np.flatnonzero(frames["channel"] == a):
                for j in np.flatnonzero((sc.nd.channel == b) & (sc.nd.enabled != 0)):
                    if S.rssi_of(O, sc, frames[k:k + 1], j) >= sc.model(O).ld_sensitivity_dbm:
                        found = True
                        break
                if found:
                    break
            assert found, (a, b)
    # and no link crosses channels
    assert (frames["channel"][exp.pkt] == sc.nd.channel[exp.dst]).all()


def test_bounds_every_exact_next_pair_differs_at_the_chosen_link(O):
    base = S.run(O, "bounds/base").exp[0]
    for which in S.BOUNDS:
        k, v = S.bounds_link(O, which)
        pkt, dst = int(base.pkt[k]), int(base.dst[k])
        ex, nx = S.run(O, "bounds/%s/exact" % which).exp[0], S.run(O, "bounds/%s/next" % which).exp[0]
        le, ln = _links(ex), _links(nx)
        assert (pkt, dst) in le, which                    # at its own value the link is heard
        if which == "sensitivity":
            assert ex.rssi[le[(pkt, dst)]] == v
            # the next double drops this link and what has the very same rssi (the reverse link: E2 is symmetric), nothing else
            gone = set(le) - set(ln)
            assert (pkt, dst) in gone and gone == {key for key, i in le.items() if ex.rssi[i] == v} and not set(ln) - set(le)
        elif which == "capture":
            assert ex.sinr[le[(pkt, dst)]] == v and ex.verdict[le[(pkt, dst)]] == O.DELIVERED
            assert nx.sinr[ln[(pkt, dst)]] == v and nx.verdict[ln[(pkt, dst)]] == O.INTERFERED
        else:
            # the chosen frame is an interferer at its receiver iff rssi >= ifloor: the OTHER frames heard there change their sinr;
            # the link itself keeps it (its own power is not part of its interference either way)
            assert ex.rssi[le[(pkt, dst)]] == v and ex.count == nx.count
            assert ex.sinr[le[(pkt, dst)]] == nx.sinr[ln[(pkt, dst)]]
            others = [key for key in le if key[1] == dst and key[0] != pkt]
            assert others and all(ex.sinr[le[key]] < nx.sinr[ln[key]] for key in others), which
            same = [key for key in le if key[1] != dst]
            assert all(ex.sinr[le[key]] == nx.sinr[ln[key]] for key in same)


def test_everyone_half_duplex_with_air_time_and_none_without(O):
    for n in (64, 65):
        sc, r = S.scene(O, "everyone/%d" % n), S.run(O, "everyone/%d" % n)
        on, off, one = r.exp
        assert on.count == off.count == n * (n - 1) and one.count == n - 1
        assert (on.verdict == O.INTERFERED).all()
        assert (r.alone(0).verdict == O.INTERFERED).all() and len(r.before[0]) == 0
        # air 0: nothing overlaps, no receiver is on the air: sinr = rssi - noise, every link delivered, no packet marked
        noise = 10.0 * O.lib().orc_det_log10(O.lib().orc_det_pow10(sc.model(O).ld_noise_dbm / 10.0))
        assert np.array_equal(off.sinr, off.rssi - noise) and (off.verdict == O.DELIVERED).all()
        assert not off.pkt_interference.any() and not on.pkt_interference.any()
        assert np.array_equal(one.sinr, one.rssi - noise)          # one frame: the sum less the link's own power is 0
        # with air time, and capture out of the way, half duplex alone interferes every link
        relaxed = O.tick(O.model(O.MODEL_LOGDIST, **dict(sc.params, ld_capture_db=-1000.0)), sc.nd, r.new[0])
        assert (relaxed.verdict == O.INTERFERED).all()


def test_quiet_every_term_is_zero(O):
    for name in S.FAMILIES["quiet"]:
        sc, r = S.scene(O, name), S.run(O, name)
        mdl = sc.model(O)
        noise = 10.0 * O.lib().orc_det_log10(O.lib().orc_det_pow10(mdl.ld_noise_dbm / 10.0))
        for k, exp in enumerate(r.exp):
            n_new = len(r.new[k])
            assert exp.count == n_new * (sc.nd.n - 1)              # every frame is heard by every other node ...
            assert (exp.rssi >= mdl.ld_ifloor_dbm).all()           # ... and is an interferer there (a term exists) ...
            lin = np.array([O.lib().orc_det_pow10(v / 10.0) for v in np.unique(exp.rssi)])
            assert (lin > 0).all() and all(S.R.to_fixed(float(v)) == 0 for v in lin)      # ... whose Q80 value is 0
            assert np.array_equal(exp.sinr, exp.rssi - noise)
        # both verdicts among the links whose receiver does not transmit
        exp = r.exp[0]
        idle = ~np.isin(exp.dst, sc.ticks[0].src)
        if name != "quiet/coincident":
            assert {O.INTERFERED, O.DELIVERED} <= set(exp.verdict[idle].tolist()), name
        else:       # sinr == capture on every link: delivered unless the receiver is on the air
            assert (exp.sinr == sc.params["ld_capture_db"]).all() and (exp.verdict[idle] == O.DELIVERED).all()
            assert (exp.verdict[~idle] == O.INTERFERED).all() and (~idle).any()
    a, b = S.run(O, "quiet/clip0").exp[0], S.run(O, "quiet/clip1").exp[0]
    assert not np.array_equal(a.rssi, b.rssi)                      # clip 0 takes the shadowing out, clip 1 leaves some


def test_tiny_tables(O):
    r1, r2, r3, re_ = (S.run(O, "tiny/" + w) for w in ("1", "2", "3", "empty"))
    assert [e.count for e in r1.exp] == [0, 0, 0] and r1.tail(r1.sc.end())[1].count == 0
    assert [e.count for e in r2.exp] == [2, 1, 1] and (r2.exp[0].verdict == O.INTERFERED).all() and (r2.exp[1].verdict == O.DELIVERED).all()
    assert r2.tail(r2.sc.end())[2] == 1                                  # the last frame is still on the air for the tail tick
    assert [e.count for e in r3.exp] == [2, 0, 0, 2] and len(r3.new[1]) == 1 and len(r3.new[2]) == 0      # a frame nobody receives, an empty tick
    assert all(len(n) == 0 for n in re_.new) and re_.tail(re_.sc.end())[1].count > 0


def test_spans_one_microsecond_and_the_frames_without_air_time(O):
    base, moved = S.run(O, "spans/base"), S.run(O, "spans/moved")
    sc = base.sc
    names = [s[0] for s in S.SPANS]
    recs = base.new[0]
    assert (recs["start_us"] + recs["air_us"] <= sc.ticks[0].t_end).all() and (recs["start_us"] >= 0).all()
    eb, em = base.exp[0], moved.exp[0]
    assert eb.count == em.count and np.array_equal(eb.rssi, em.rssi)
    assert (eb.sinr != em.sinr).any()                                    # abutting -> overlapping by 1 us

    def without(name):
        keep = np.array([n != name for n in names])
        res = O.tick(base.mdl, sc.nd, recs[keep])
        full = np.isin(eb.pkt, np.flatnonzero(keep))
        return res, full
    # the air-0 frame at the tick's begin interferes with nothing: without it every other link is what it was
    res, full = without("zero_at_begin")
    assert np.array_equal(res.sinr, eb.sinr[full]) and np.array_equal(res.verdict, eb.verdict[full])
    # ... and nothing interferes with it
    z = eb.pkt == names.index("zero_at_begin")
    noise = 10.0 * O.lib().orc_det_log10(O.lib().orc_det_pow10(base.mdl.ld_noise_dbm / 10.0))
    assert z.any() and np.array_equal(eb.sinr[z], eb.rssi[z] - noise)
    # the air-0 frame strictly inside other spans does interfere (E3's overlap test holds for it)
    res, full = without("zero_inside")
    assert (res.sinr != eb.sinr[full]).any()
    # half duplex by time: twin_a's link to the source of `near` (spans overlap) is interfered whatever its sinr, its link to the
    # source of `later` (no overlap) is not half duplex
    relaxed = O.tick(O.model(O.MODEL_LOGDIST, **dict(sc.params, ld_capture_db=-1000.0)), sc.nd, recs)
    lk = _links(relaxed)
    a = names.index("twin_a")
    assert relaxed.verdict[lk[(a, sc.who["near"])]] == O.INTERFERED
    assert relaxed.verdict[lk[(a, sc.who["later"])]] == O.DELIVERED
    # per-frame power and channel differ from the table's
    assert (recs["txpower"] != sc.nd.txpower[recs["src"]]).sum() == 2 and (recs["channel"] != sc.nd.channel[recs["src"]]).sum() == 1
    inner = eb.pkt == names.index("inner")
    assert inner.any() and (sc.nd.channel[eb.dst[inner]] == 11).all()


def test_chain_earlier_ticks_decide_verdicts_and_receivers_are_on_the_air(O):
    sc, r = S.scene(O, "chain"), S.run(O, "chain")
    assert [len(t) for t in sc.ticks] == S.CHAIN_SIZES and sc.nd.n == 257
    assert set(S.CHAIN_AIRS) == {0, 300, 999, 1000, 1001, 8128, 20000}
    assert len(np.unique(sc.nd.channel)) == 3 and sc.params["ld_sigma_db"] > 0
    owed, half = 0, 0
    for k, exp in enumerate(r.exp):
        if not exp.count:
            continue
        alone = r.alone(k)
        assert alone.count == exp.count
        owed += int(((exp.verdict == O.INTERFERED) & (alone.verdict == O.DELIVERED)).sum())
        # a node that transmitted in tick k - 1, still on the air, hears a frame of tick k that overlaps its own
        if k > 0 and len(r.new[k - 1]):
            prev = r.new[k - 1]
            new = r.new[k]
            for p, d in zip(exp.pkt, exp.dst):
                m = prev["src"] == d
                if m.any():
                    e = int(prev["start_us"][m][0] + prev["air_us"][m][0])
                    if e > new["start_us"][p] and prev["start_us"][m][0] < new["start_us"][p] + new["air_us"][p]:
                        half += 1
    assert owed > 100 and half > 10, (owed, half)
    # the verdicts after the big ticks are not all the same
    assert sum(int((e.verdict == O.DELIVERED).sum()) for e in r.exp[8:]) > 50
    # frames that end exactly where the next tick's frames start do not overlap them: one microsecond more and they do
    for k in S.CHAIN_ENDS_AT_NEXT:
        assert S.CHAIN_AIRS[k] == S.TICK and S.CHAIN_SIZES[k] and S.CHAIN_SIZES[k + 1]
        assert sc.ticks[k].start + S.CHAIN_AIRS[k] == sc.ticks[k + 1].start
        airs = list(S.CHAIN_AIRS)
        airs[k] += 1
        longer = S.Run(O, S.chain(O, airs)).exp[k + 1]
        assert longer.count == r.exp[k + 1].count
        assert (longer.sinr != r.exp[k + 1].sinr).any() and (longer.verdict != r.exp[k + 1].verdict).any(), k
    assert len(r.before[16]) > len(r.before[15]) and sc.ticks[16].start > sc.ticks[16].t_begin      # tick 15's frames are on the air for tick 16
    # every cut of the chain into two batches has frames on the air at the cut
    for cut in S.CHAIN_CUTS:
        assert len(r.before[cut]) > 0
