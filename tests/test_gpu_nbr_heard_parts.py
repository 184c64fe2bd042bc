"""The heard form's record copies in spans, and the tick in which every frame is served.  The served copy
(k_reorder_served_batch) and the fill (k_nc_fill_batch) take the records of a wave's 64 consecutive frames with full lanes, a span
of 256 records at a time (sharing the spans among 2, 4 or 8 waves was measured and dropped; the span counts below keep the
boundaries such a split would have); the claim (k_nc_claim_batch) and all but one workgroup of the reorder stage leave an all-served tick at
once.  Nothing of it may show in the results: every tick of every batch here is held to the oracle bit for bit (heard set, order,
rssi, verdict, batch_result_count), in both filter shapes, and every case asserts from the oracle's own per-packet counts that
the situation it is about really occurs in its scene.  No draw can happen in any scene (no rxprob below 1, txprob 0 or 1), so a
tick's oracle result is computed once and holds for every repetition."""
import numpy as np
import pytest

from util import configure_engine, oracle_model, random_nodes, assert_same, DeviceArray

pytestmark = pytest.mark.gpu

AIR = 8128
SPAN = 256          # records a wave takes at a time (kCopySpan, rm_device.hpp)
PARTS = (1, 2, 4, 8)  # span counts whose boundaries are covered: totals of SPAN * P and SPAN * P * 2, and one to either side

_SCENES = {}        # a case's scene and its oracle results: built once, shared by the two filter shapes, left unchanged


@pytest.fixture(autouse=True, params=[None, "2"], ids=["", "near-lists"])
def near_lists(request, monkeypatch):
    """Every case twice, as in test_gpu_nbr_heard.py: the filter the sizes here choose, and the 1024-receiver workgroups with the
    near-frame lists that the bench shape takes."""
    if request.param:
        monkeypatch.setenv("RM_NEAR_LISTS", request.param)
        monkeypatch.setenv("RM_WG_RPT", "4")


def _layout(O, n, seed):
    return random_nodes(O, n, 50.0 * np.sqrt(np.pi * n / 20.0), seed=seed)


def _oracle(O, mdl, nd, srcs):
    """the oracle's result of every tick of a launch sequence over `srcs` (start times as _run gives them)"""
    return [O.tick(mdl, nd, nd.packets(s, start_us=1000 * b, air_us=AIR)) for b, s in enumerate(srcs)]


def _run(engine, srcs):
    dev = [DeviceArray(s) for s in srcs]
    starts = [1000 * b for b in range(len(srcs))]
    engine.batch_run_sources_device(starts, [s + 1000 for s in starts], [d.ptr.value for d in dev], [len(s) for s in srcs], starts,
                                    [AIR] * len(srcs))
    for d in dev:
        d.free()


def _batch(engine, srcs, want, what):
    """one launch sequence over the ticks `srcs`, every tick against its oracle result"""
    _run(engine, srcs)
    for b, s in enumerate(srcs):
        assert_same(engine.batch_result_copy(b, len(s)), want[b], "%s, tick %d" % (what, b))
        assert engine.batch_result_count(b) == (want[b].count, 0), (what, b)


def _swept(engine, n_slots):
    """per slot: the candidates the sweep handed to the exact stage (0: every frame of the tick was served from a list)"""
    return [engine.slot_stats(b)[0] for b in range(n_slots)]


def _per_pkt(w, n_frames):
    return np.bincount(w.pkt, minlength=n_frames)[:n_frames]


def _group_totals(w, n_frames):
    """heard links of the 64-frame groups of a tick (frames 64 g .. 64 g + 63 in tick order): what one wave copies"""
    c = _per_pkt(w, n_frames)
    return [int(c[g:g + 64].sum()) for g in range(0, n_frames, 64)]


def _sample(n, n_ticks, per_tick, seed, among=None):
    rng = np.random.default_rng(seed)
    pool = np.arange(n) if among is None else np.asarray(among)
    return [np.sort(rng.choice(pool, per_tick, replace=False)).astype(np.int32) for _ in range(n_ticks)]


# ---- 1. part boundaries ------------------------------------------------------------------------------------------------------------

GRID, STEP, EDGE = 78, 50.0, 5      # 78 x 78 nodes 50 m apart; sources keep 5 steps from the border (the largest reach is 4.7)
# reach in steps -> lattice points inside it (the source itself not counted): every interior source of one power hears exactly that many
REACH = {0.5: 0, 1.2: 4, 1.7: 8, 2.1: 12, 2.5: 20, 2.9: 24, 3.1: 28, 3.4: 36, 3.8: 44, 4.05: 48, 4.2: 56, 4.35: 60, 4.7: 68}
# group totals asked for: nothing, less than a span, and every multiple of the span that is 256 * P or 256 * P * 2 for an allowed P,
# with the totals one below and one above
TARGETS = [0, 100] + [m * SPAN + d for m in (1, 2, 4, 8, 16) for d in (-1, 0, 1)]


def _compose(total, pool, n=64):
    """n unused sources of `pool` (heard count -> sources) whose counts add up to `total`: one of count c0, x of count a, the
    others of count b.  The sources are taken out of the pool."""
    vals = sorted(v for v in pool if pool[v])
    for c0 in vals:
        for a in vals:
            for x in range(n - 1):
                rest, m = total - c0 - x * a, n - 1 - x
                if rest < 0 or rest % m or rest // m not in pool:
                    continue
                need = {}
                for v, k in ((c0, 1), (a, x), (rest // m, m)):
                    need[v] = need.get(v, 0) + k
                if all(len(pool[v]) >= k for v, k in need.items()):
                    return [pool[v].pop() for v, k in need.items() for _ in range(k)]
    raise AssertionError("no 64 sources left whose heard counts add up to %d" % total)


def _lattice_scene(O):
    if "lattice" in _SCENES:
        return _SCENES["lattice"]
    n = GRID * GRID
    rng = np.random.default_rng(7)
    nd = O.NodeTable(n)
    row, col = np.divmod(np.arange(n), GRID)
    nd.x, nd.y = col * STEP, row * STEP
    # per-source power: rssi = txpower - 40 - 30 log10(d) against a sensitivity of -95 dBm (the medium's defaults), sigma 0
    reach = np.array(sorted(REACH))
    p = np.ones(len(reach))
    p[0] = 3.0          # (the groups without a record and with less than a span of them are made of silent sources ...
    p[-4:] = 2.0        # ... and three groups of 16 spans of the loudest ones)
    nd.txpower = 30.0 * np.log10(STEP * reach[rng.choice(len(reach), n, p=p / p.sum())]) - 55.0
    interior = (row >= EDGE) & (row < GRID - EDGE) & (col >= EDGE) & (col < GRID - EDGE)
    # a few receivers switched off: the sources around one hear one node less -- totals that are no multiple of 4
    off = rng.choice(np.flatnonzero(interior), 24, replace=False)
    nd.enabled[off] = 0
    params = dict(ld_sigma_db=0.0)
    mdl = oracle_model(O, "logdist", params)
    cand = np.flatnonzero(interior & (nd.enabled == 1)).astype(np.int32)
    count = _per_pkt(O.tick(mdl, nd, nd.packets(cand, start_us=0, air_us=AIR)), len(cand))
    assert set(REACH.values()) <= set(count.tolist()) and (count % 4 != 0).sum() > 100   # the lattice counts, and odd ones
    # tick order is node order, so group g of a tick takes its sources from the g-th band of rows: sorting a tick keeps its groups
    rows = GRID - 2 * EDGE
    band = np.minimum((row[cand] - EDGE) * 4 // rows, 3)
    pools = [{} for _ in range(4)]
    for s, c, b in zip(cand.tolist(), count.tolist(), band.tolist()):
        pools[b].setdefault(c, []).append(s)
    targets = TARGETS + [None] * (-len(TARGETS) % 4)
    srcs = []
    for t0 in range(0, len(targets), 4):
        tick = []
        for g, total in enumerate(targets[t0:t0 + 4]):
            if total is None:   # (a group to fill the tick: the loudest sources left in the band)
                left = [s for v in sorted(pools[g]) for s in pools[g][v]]
                tick += left[-64:]
            else:
                tick += _compose(total, pools[g])
        srcs.append(np.sort(np.array(tick, dtype=np.int32)))
    assert all(len(s) == 256 == len(np.unique(s)) for s in srcs) and len(np.unique(np.concatenate(srcs))) == 256 * len(srcs)
    want = _oracle(O, mdl, nd, srcs)
    _SCENES["lattice"] = (nd, params, srcs, want)
    return _SCENES["lattice"]


def test_part_boundaries(engine, rsa, O):
    """Group totals of 0, below a span, at 256 * {1, 2, 4, 8, 16} and one record to either side: the last span of a group is
    full, holds one record, or lacks one; a group has no span at all, one, or several.  Filled (the fill's copy), then served twice (the served copy)."""
    nd, params, srcs, want = _lattice_scene(O)
    totals = set(t for w, s in zip(want, srcs) for t in _group_totals(w, len(s)))
    assert set(TARGETS) <= totals, sorted(set(TARGETS) - totals)
    for parts in PARTS:
        assert {SPAN * parts, SPAN * parts - 1, SPAN * parts + 1, SPAN * parts * 2} <= totals
    assert 4 <= len(srcs) <= 6
    configure_engine(engine, nd, "logdist", params)
    for rep in range(3):
        _batch(engine, srcs, want, "lattice, batch %d" % rep)
        swept = _swept(engine, len(srcs))
        assert all((c > 0) == (rep == 0) for c in swept), (rep, swept)


# ---- 2. ragged ticks in one batch --------------------------------------------------------------------------------------------------

RAGGED = (1, 63, 64, 65, 150, 300)


def _ragged_scene(O):
    if "ragged" in _SCENES:
        return _SCENES["ragged"]
    n = 6000
    nd = _layout(O, n, seed=71)
    params = dict(ld_sigma_db=4.0, ld_seed=13)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(72).permutation(n)
    sets, at = [], 0
    for k in range(3):      # three disjoint families of ticks of the ragged sizes
        fam = []
        for m in RAGGED:
            fam.append(np.sort(ids[at:at + m]).astype(np.int32))
            at += m
        sets.append(fam)
    a, b, c = sets
    seqs = [a,                                                   # cold
            [a[0], b[1], a[2], b[3], a[4], b[5]],                # served and swept ticks side by side
            [c[0], b[1], c[2], b[3], c[4], b[5]]]                # the other way round: every size both served and swept
    served = [[False] * 6, [True, False] * 3, [False, True] * 3]
    want = [_oracle(O, mdl, nd, s) for s in seqs]
    _SCENES["ragged"] = (nd, params, seqs, served, want)
    return _SCENES["ragged"]


def test_ragged_ticks(engine, rsa, O):
    """Ticks of 1, 63, 64, 65, 150 and 300 frames in one launch sequence: the grid is sized by the largest, so the small ticks
    have waves and whole workgroups beyond their frames; an all-served tick sits beside an all-swept one."""
    nd, params, seqs, served, want = _ragged_scene(O)
    for srcs, w in zip(seqs, want):
        assert tuple(len(s) for s in srcs) == RAGGED
        assert all(x.count > 0 for x in w)          # every tick, the one-frame ticks included, has records to place
    configure_engine(engine, nd, "logdist", params)
    for srcs, sv, w, what in zip(seqs, served, want, ("cold", "served / swept", "swept / served")):
        _batch(engine, srcs, w, what)
        swept = _swept(engine, len(srcs))
        assert [c == 0 for c in swept] == sv, (what, swept)
    _batch(engine, seqs[2], want[2], "all served")
    assert _swept(engine, 6) == [0] * 6


# ---- 3. stale fill words -----------------------------------------------------------------------------------------------------------

def _stale_scene(O):
    if "stale" in _SCENES:
        return _SCENES["stale"]
    n = 6000
    nd = _layout(O, n, seed=81)
    params = dict(ld_sigma_db=2.0, ld_seed=3)
    mdl = oracle_model(O, "logdist", params)
    base = _sample(n, 4, 200, seed=82)
    fresh = np.setdiff1d(np.arange(n), np.concatenate(base))
    extra = _sample(n, 4, 7, seed=83, among=fresh)
    assert len(np.unique(np.concatenate(extra))) == 28
    more = [np.sort(np.concatenate([s, x])).astype(np.int32) for s, x in zip(base, extra)]
    _SCENES["stale"] = (nd, params, base, more, extra, _oracle(O, mdl, nd, base), _oracle(O, mdl, nd, more))
    return _SCENES["stale"]


def test_stale_fill_words(engine, rsa, O):
    """fill[] is not cleared between launch sequences and the claim of an all-served tick writes nothing.  Sequence 1 claims for
    every frame, sequence 2 serves every frame, sequence 3 adds a few never-seen sources at scattered places: their lists must
    be filled from THEIR frames of sequence 3 -- sequence 4 serves them, against the oracle, with nothing swept."""
    nd, params, base, more, extra, want_base, want_more = _stale_scene(O)
    for s, x, w in zip(more, extra, want_more):
        at = np.searchsorted(s, x)                  # the new frames' places in the tick: every frame behind one has moved
        assert at.min() < 64 and at.max() >= 128 and len(np.unique(at // 64)) >= 3, at      # scattered over the waves
        assert (_per_pkt(w, len(s))[at] > 0).all()                                          # each with records to keep
    configure_engine(engine, nd, "logdist", params)
    _batch(engine, base, want_base, "sequence 1 (cold)")
    assert all(c > 0 for c in _swept(engine, 4))
    _batch(engine, base, want_base, "sequence 2 (all served)")
    assert _swept(engine, 4) == [0] * 4
    _batch(engine, more, want_more, "sequence 3 (new sources among served ones)")
    swept = _swept(engine, 4)
    assert all(c > 0 for c in swept), swept
    _batch(engine, more, want_more, "sequence 4 (all served)")
    assert _swept(engine, 4) == [0] * 4


# ---- 4. an all-served tick among swept ticks ---------------------------------------------------------------------------------------

def _among_scene(O):
    if "among" in _SCENES:
        return _SCENES["among"]
    n = 6000
    nd = _layout(O, n, seed=91)
    ids = np.random.default_rng(92).permutation(n)
    known = [np.sort(ids[k * 220:(k + 1) * 220]).astype(np.int32) for k in range(4)]
    new = [np.sort(ids[2000 + k * 180:2000 + (k + 1) * 180]).astype(np.int32) for k in range(2)]
    nd.txprob[np.concatenate([s[::3] for s in known + new])] = 0.0     # the Tx-failure flag is not constant
    params = dict(ld_sigma_db=4.0, ld_seed=17)
    mdl = oracle_model(O, "logdist", params)
    mixed = [known[0], new[0], known[2], new[1]]
    _SCENES["among"] = (nd, params, known, mixed, _oracle(O, mdl, nd, known), _oracle(O, mdl, nd, mixed))
    return _SCENES["among"]


def test_all_served_tick_among_swept_ticks(engine, rsa, O):
    """Ticks 0 and 2 repeat known sources only, ticks 1 and 3 hold only new ones.  The claim and all but one reorder workgroup of
    ticks 0 and 2 return early: their share of pkt_interference and the packets' offsets (the records' packet numbers) must be
    right all the same -- assert_same compares both, read through batch_result_copy."""
    nd, params, known, mixed, want_known, want_mixed = _among_scene(O)
    for b in (0, 2):
        flags = np.asarray(want_mixed[b].pkt_interference)[:len(mixed[b])]
        assert 0 < int((flags != 0).sum()) < len(flags)             # both values of the flag in the served ticks
        assert want_mixed[b].count > 0 and len(mixed[b]) > 64 * 3   # more workgroups than the publisher share the flags
    configure_engine(engine, nd, "logdist", params)
    _batch(engine, known, want_known, "warm")
    _batch(engine, mixed, want_mixed, "served ticks among swept ones")
    swept = _swept(engine, 4)
    assert swept[0] == 0 and swept[2] == 0 and swept[1] > 0 and swept[3] > 0, swept
    _batch(engine, mixed, want_mixed, "all served")
    assert _swept(engine, 4) == [0] * 4


# ---- 5. capacity -------------------------------------------------------------------------------------------------------------------

def _capacity_scene(O):
    if "capacity" in _SCENES:
        return _SCENES["capacity"]
    # the scene of test_gpu_nbr_heard.py::test_dropped_ticks_leave_no_list with 300 instead of 150 frames per tick and 300 loud
    # sources instead of 200
    n = 6000
    nd = _layout(O, n, seed=41)
    params = dict(ld_sigma_db=0.0)
    mdl = oracle_model(O, "logdist", params)
    small = _sample(n, 4, 300, seed=42)
    loud = np.setdiff1d(_sample(n, 1, 400, seed=43)[0], np.concatenate(small))[:300].astype(np.int32)
    nd.txpower[np.concatenate(small)] = -14.0
    nd.txpower[loud] = 10.0
    big = np.unique(np.concatenate([small[0][::2], small[2][::2], loud])).astype(np.int32)
    srcs = [small[0], small[1], big, small[2], small[3]]
    _SCENES["capacity"] = (nd, params, srcs, loud, _oracle(O, mdl, nd, srcs))
    return _SCENES["capacity"]


def test_capacity(engine, rsa, O):
    """A link capacity below one tick's heard total, with groups of more than 256 * 8 records in that tick: the tick is dropped
    in both runs, its records stop at the capacity under the full-lane copy -- served frames on either side of it --, it leaves no
    list; with room again the batch equals the oracle twice (the loud sources swept and filled, then served)."""
    nd, params, srcs, loud, want = _capacity_scene(O)
    cap = 1 << 15
    assert 20 * max(w.count for b, w in enumerate(want) if b != 2) < cap < want[2].count
    assert max(_group_totals(want[2], len(srcs[2]))) > SPAN * max(PARTS)
    # the dropped tick's frames that are served in the second run (half of ticks 0 and 3's sources): records below and beyond `cap`
    off = np.concatenate([[0], np.cumsum(_per_pkt(want[2], len(srcs[2])))])
    quiet = np.flatnonzero(~np.isin(srcs[2], loud))
    has = quiet[off[quiet + 1] > off[quiet]]
    assert (off[has + 1] <= cap).any() and (off[has] >= cap).any()
    configure_engine(engine, nd, "logdist", params)
    engine.set_link_capacity(cap)
    for rep in range(2):
        _run(engine, srcs)
        for b, s in enumerate(srcs):
            cnt, dropped = engine.batch_result_count(b)
            assert dropped == (1 if b == 2 else 0), (rep, b)
            if b != 2:
                assert_same(engine.batch_result_copy(b, len(s)), want[b], "small capacity, batch %d, tick %d" % (rep, b))
        swept = _swept(engine, len(srcs))
        assert swept[2] > 0 and all((c > 0) == (rep == 0) for b, c in enumerate(swept) if b != 2), (rep, swept)
    engine.set_link_capacity(1 << 20)
    for rep in range(2):
        _batch(engine, srcs, want, "room again, batch %d" % rep)
        swept = _swept(engine, len(srcs))
        # the dropped tick left no list: its loud sources are swept once more; the lists of the others outlived both capacities
        assert (swept[2] > 0) == (rep == 0) and all(c == 0 for b, c in enumerate(swept) if b != 2), (rep, swept)
    # The capacity lowered again (rm_set_link_capacity leaves the lists): the big tick is served whole now, nothing of it is staged,
    # and its total alone is beyond the capacity -- the served copy itself runs into `cap` (its `o < cap` guard cuts the frame
    # that straddles it and all behind it; served frames lie on either side of the cut, asserted above from `off`).  The tick is
    # reported dropped with its full total and no reader hands out its records; the ticks around it are the oracle's.
    engine.set_link_capacity(cap)
    _run(engine, srcs)
    assert _swept(engine, len(srcs)) == [0] * len(srcs)
    for b, s in enumerate(srcs):
        cnt, dropped = engine.batch_result_count(b)
        assert (cnt, dropped) == (want[b].count, 1 if b == 2 else 0), (b, cnt, dropped)
        if b != 2:
            assert_same(engine.batch_result_copy(b, len(s)), want[b], "all served, small capacity, tick %d" % b)
        else:
            with pytest.raises(rsa.RadioMediumError, match="link capacity"):
                engine.batch_result_copy(b, len(s))
    engine.set_link_capacity(1 << 20)
    _batch(engine, srcs, want, "room once more")   # the dropped tick's lists are as they were: still served, still right
    assert _swept(engine, len(srcs)) == [0] * len(srcs)
