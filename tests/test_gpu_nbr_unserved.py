"""The heard form's list of unserved frames: in a tick that has hits the pre-pass lists the frames WITHOUT one
(n_un of them, the ones that reach nobody included), the reorder stage walks that list instead of the tick's frames -- a
workgroup whose first position lies beyond it leaves before the scan --, and the claim and the fill take one list position per
thread and per lane, with fill[] kept by position.  A tick without any hit has no list to follow.  Nothing of it may show in the
results: every tick of every batch here is held to the oracle bit for bit (heard set, order, rssi, verdict,
batch_result_count), in both filter shapes, and every case asserts from its own construction and from the oracle's per-packet
counts that the situation it is about really occurs.  A source that has not transmitted since the table was uploaded has no
list, one that has (in a tick that was not dropped) is served: that is how the cases place their unserved frames.  Apart from
test_form_switch no draw can happen (no rxprob below 1, txprob 0 or 1), so a tick's oracle result is computed once per scene."""
import numpy as np
import pytest

from util import configure_engine, oracle_model, random_nodes, assert_same, DeviceArray

pytestmark = pytest.mark.gpu

AIR = 8128
N = 6000

_SCENES = {}        # a case's scene and its oracle results: built once, shared by the cases that run it, left unchanged


@pytest.fixture(autouse=True, params=[None, "2"], ids=["", "near-lists"])
def near_lists(request, monkeypatch):
    """Every case twice, as in test_gpu_nbr_heard_parts.py: the filter the sizes here choose, and the 1024-receiver workgroups
    with the near-frame lists that the bench shape takes."""
    if request.param:
        monkeypatch.setenv("RM_NEAR_LISTS", request.param)
        monkeypatch.setenv("RM_WG_RPT", "4")


def _layout(O, seed):
    return random_nodes(O, N, 50.0 * np.sqrt(np.pi * N / 20.0), seed=seed)


def _oracle(O, mdl, nd, srcs):
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
    """per slot: the candidates the sweep handed to the exact stage (0: no frame of the tick was swept)"""
    return [engine.slot_stats(b)[0] for b in range(n_slots)]


def _per_pkt(w, n_frames):
    return np.bincount(w.pkt, minlength=n_frames)[:n_frames]


def _merge(*parts):
    s = np.sort(np.concatenate(parts)).astype(np.int32)
    assert len(np.unique(s)) == len(s)
    return s


# ---- 1. boundaries of n_un ---------------------------------------------------------------------------------------------------------

FRAMES = 250
COUNTS = (0, 1, 3, 12, 13, 64, 65, FRAMES)      # unserved frames of the second batch's ticks


def _places(place, m):
    """the positions of a tick's m unserved frames"""
    if m == FRAMES:
        return np.arange(FRAMES)
    if place == "start":
        return np.arange(m)
    if place == "end":
        return np.arange(FRAMES - m, FRAMES)
    if m == 1:
        return np.array([130])
    at = np.unique(np.round(np.linspace(2, FRAMES - 3, m)).astype(int))
    assert len(at) == m
    return at


def _counts_scene(O, place):
    key = ("counts", place)
    if key in _SCENES:
        return _SCENES[key]
    nd = _layout(O, seed=101)
    params = dict(ld_sigma_db=4.0, ld_seed=19)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(102).permutation(N)
    ticks = [np.sort(ids[b * FRAMES:(b + 1) * FRAMES]).astype(np.int32) for b in range(len(COUNTS))]
    spare = np.sort(ids[len(COUNTS) * FRAMES:(len(COUNTS) + 1) * FRAMES]).astype(np.int32)
    at = [_places(place, m) for m in COUNTS]
    warm = [np.delete(t, p) if len(p) < FRAMES else spare for t, p in zip(ticks, at)]   # (the last tick's sources are all new)
    _SCENES[key] = (nd, params, warm, ticks, at, _oracle(O, mdl, nd, warm), _oracle(O, mdl, nd, ticks))
    return _SCENES[key]


@pytest.mark.parametrize("fpw", ["3", "1", "200"])
@pytest.mark.parametrize("place", ["start", "end", "scattered"])
def test_unserved_counts(engine, rsa, O, monkeypatch, place, fpw):
    """One batch warms the lists; the second one's ticks have 0, 1, 3, 12, 13, 64, 65 and every one of their 250 frames unserved
    -- at the tick's start, at its end, or scattered over its waves.  RM_FPW=3: twelve positions per reorder workgroup, 1: four,
    200: one workgroup, the publisher, does all the work.  The third batch is served whole."""
    monkeypatch.setenv("RM_FPW", fpw)
    nd, params, warm, ticks, at, want_warm, want = _counts_scene(O, place)
    assert tuple(len(p) for p in at) == COUNTS
    for t, p, w, x in zip(ticks, at, want, warm):
        assert len(t) == FRAMES and len(np.intersect1d(t[p], np.concatenate(warm))) == 0     # the unserved frames' sources are new
        assert len(p) == FRAMES or np.array_equal(np.delete(t, p), x)                        # ... and every other one is known
        assert len(p) == 0 or (_per_pkt(w, FRAMES)[p] > 0).all()                             # each with records to rank and keep
        if place == "scattered" and len(p) >= 3:
            assert len(np.unique(p // 64)) >= 3, p
    configure_engine(engine, nd, "logdist", params)
    _batch(engine, warm, want_warm, "warm")
    assert all(c > 0 for c in _swept(engine, len(warm)))
    _batch(engine, ticks, want, "unserved %s, RM_FPW=%s" % (place, fpw))
    swept = _swept(engine, len(ticks))
    assert [c > 0 for c in swept] == [m > 0 for m in COUNTS], swept
    _batch(engine, ticks, want, "all served")
    assert _swept(engine, len(ticks)) == [0] * len(ticks)


# ---- 2. sources that reach nobody --------------------------------------------------------------------------------------------------

def _silent_scene(O):
    if "silent" in _SCENES:
        return _SCENES["silent"]
    nd = _layout(O, seed=111)
    params = dict(ld_sigma_db=2.0, ld_seed=5)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(112).permutation(N)
    known = [ids[b * 150:(b + 1) * 150] for b in range(3)]
    pool = ids[1000:]
    # (-30 dBm still reaches a node within a few metres: of 400 such sources, those for which the oracle finds no link at all)
    quiet = np.sort(pool[600:1000]).astype(np.int32)
    nd.txpower[quiet] = -30.0
    quiet = quiet[_per_pkt(O.tick(mdl, nd, nd.packets(quiet, start_us=0, air_us=AIR)), len(quiet)) == 0]
    assert len(quiet) >= 120
    # (30 per tick, evenly over the whole range of node numbers: all over their ticks)
    silent = [quiet[b::4][np.linspace(0, len(quiet[b::4]) - 1, 30).astype(int)] for b in range(4)]
    long1 = [pool[200 + b * 6:200 + (b + 1) * 6] for b in range(4)]      # more than 64 records
    long2 = [pool[300 + b * 4:300 + (b + 1) * 4] for b in range(4)]      # more than 256
    plain = [pool[400 + b * 20:400 + (b + 1) * 20] for b in range(4)]
    # (... and sources below the medium's cut-off at any distance: the pre-pass itself finds that they reach nobody)
    mute = pool[1100:1130]
    nd.txpower[mute] = -80.0
    nd.txpower[np.concatenate(long1)] = 8.0
    nd.txpower[np.concatenate(long2)] = 15.0
    warm = [_merge(k) for k in known]
    mixed = [_merge(known[0], mute),                                     # unserved frames, and none of them for the sweep
             _merge(known[1], silent[1], long1[1], long2[1], plain[1]),
             _merge(known[2], silent[2], long1[2], long2[2]),            # long frames beside silent ones
             _merge(silent[3], long1[3], long2[3], plain[3])]            # no hit at all: no list to follow
    silent[0] = np.sort(mute)
    _SCENES["silent"] = (nd, params, warm, mixed, silent, _oracle(O, mdl, nd, warm), _oracle(O, mdl, nd, mixed))
    return _SCENES["silent"]


def test_sources_that_reach_nobody(engine, rsa, O):
    """Unserved frames with txpower -30 have no heard link: they sit in the list, claim an empty list and are served, with
    nothing swept, in the next batch (the sweep still looks at them: a node might have stood within their few metres).  Frames of
    more than 64 and more than 256 records sit beside them.  Tick 0's unserved frames are at -80, below the medium's cut-off at
    any distance: the pre-pass lists them and leaves none of them to the sweep -- a tick with a list and nothing swept."""
    nd, params, warm, mixed, silent, want_warm, want = _silent_scene(O)
    for b, (s, w) in enumerate(zip(mixed, want)):
        c = _per_pkt(w, len(s))
        assert len(s) <= 300 and np.isin(s, silent[b]).sum() == 30 and (c[np.isin(s, silent[b])] == 0).all()
        assert c.max() < 1024                                           # (every source can keep its list: kNcListCap)
        if b:
            assert ((c > 64) & (c <= 256)).sum() >= 3 and (c > 256).sum() >= 3, np.sort(c)[-12:]
            # silent frames and long ones among the 64 frames that were one wave's before there was a list
            groups = np.split(c, range(64, len(c), 64))
            assert any((g == 0).any() and ((g > 64) & (g <= 256)).any() for g in groups) and any((g == 0).any() and (g > 256).any() for g in groups)
    configure_engine(engine, nd, "logdist", params)
    _batch(engine, warm, want_warm, "warm")
    _batch(engine, mixed, want, "silent and long sources among known ones")
    swept = _swept(engine, len(mixed))
    assert swept[0] == 0 and all(c > 0 for c in swept[1:]), swept
    _batch(engine, mixed, want, "all served")
    assert _swept(engine, len(mixed)) == [0] * len(mixed)


# ---- 3. ragged ticks ---------------------------------------------------------------------------------------------------------------

RAGGED = (1, 63, 64, 65, 300)


def _ragged_scene(O):
    if "ragged" in _SCENES:
        return _SCENES["ragged"]
    nd = _layout(O, seed=121)
    params = dict(ld_sigma_db=4.0, ld_seed=13)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(122).permutation(N)
    fams, at = [], 0
    for k in range(4):      # four disjoint families of ticks of the ragged sizes
        fam = []
        for m in RAGGED:
            fam.append(np.sort(ids[at:at + m]).astype(np.int32))
            at += m
        fams.append(fam)
    a, b, c, d = fams

    def mix(known, new):    # every other frame known, the others new: the same size
        return _merge(known[::2], new[:len(known) - len(known[::2])])
    seqs = [a,
            [a[0], b[1], a[2], mix(a[3], b[3]), mix(a[4], b[4])],        # served | no hit at all | served | mixed | mixed
            [c[0], mix(a[1], c[1]), c[2], a[3], mix(a[4], c[4])]]        # no hit (one frame) | mixed | no hit | served | mixed
    kinds = [["cold"] * 5, ["served", "cold", "served", "mixed", "mixed"], ["cold", "mixed", "cold", "served", "mixed"]]
    _SCENES["ragged"] = (nd, params, seqs, kinds, [_oracle(O, mdl, nd, s) for s in seqs])
    return _SCENES["ragged"]


def test_ragged_ticks(engine, rsa, O):
    """Ticks of 1, 63, 64, 65 and 300 frames share one launch sequence: the grids are sized by the largest.  A tick without any
    hit (positions are frames) sits beside an all-served one and a mixed one (positions are list entries)."""
    nd, params, seqs, kinds, want = _ragged_scene(O)
    for srcs, w in zip(seqs, want):
        assert tuple(len(s) for s in srcs) == RAGGED
        assert all(x.count > 0 for x in w)
    configure_engine(engine, nd, "logdist", params)
    for srcs, kd, w, what in zip(seqs, kinds, want, ("cold", "second", "third")):
        _batch(engine, srcs, w, what)
        swept = _swept(engine, len(srcs))
        assert [c == 0 for c in swept] == [k == "served" for k in kd], (what, swept)
    _batch(engine, seqs[2], want[2], "all served")
    assert _swept(engine, len(RAGGED)) == [0] * len(RAGGED)


# ---- 4. a dropped tick -------------------------------------------------------------------------------------------------------------

def _dropped_scene(O):
    if "dropped" in _SCENES:
        return _SCENES["dropped"]
    nd = _layout(O, seed=131)
    params = dict(ld_sigma_db=0.0)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(132).permutation(N)
    small = [np.sort(ids[b * 200:(b + 1) * 200]).astype(np.int32) for b in range(4)]
    loud = np.sort(ids[1000:1100]).astype(np.int32)
    nd.txpower[np.concatenate(small)] = -14.0   # a few links per frame
    nd.txpower[loud] = 15.0
    big = _merge(small[0][::2], small[2][::2], loud)
    srcs = [small[0], small[1], big, small[2], small[3]]
    _SCENES["dropped"] = (nd, params, srcs, loud, _oracle(O, mdl, nd, srcs))
    return _SCENES["dropped"]


def test_dropped_tick(engine, rsa, O):
    """A link capacity below tick 2's heard total.  Cold, the tick is dropped with every frame unserved; in the second run two
    thirds of its frames are served and the loud third is listed, and it is dropped again: it reports dropped, leaves no list,
    and with room its loud frames are swept once more.  The other ticks equal the oracle throughout and are served from the
    second run on."""
    nd, params, srcs, loud, want = _dropped_scene(O)
    cap = 1 << 15
    assert len(srcs[2]) == 300 and 20 * max(w.count for b, w in enumerate(want) if b != 2) < cap < want[2].count
    assert _per_pkt(want[2], 300)[np.isin(srcs[2], loud)].max() < 1024
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
        assert (swept[2] > 0) == (rep == 0) and all(c == 0 for b, c in enumerate(swept) if b != 2), (rep, swept)


# ---- 5. fill by list position ------------------------------------------------------------------------------------------------------

def _position_scene(O):
    if "position" in _SCENES:
        return _SCENES["position"]
    nd = _layout(O, seed=141)
    params = dict(ld_sigma_db=2.0, ld_seed=3)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(142).permutation(N)
    base = [np.sort(ids[b * 240:(b + 1) * 240]).astype(np.int32) for b in range(4)]
    extra = [ids[2000 + b * 9:2000 + (b + 1) * 9] for b in range(4)]
    more = [_merge(s, x) for s, x in zip(base, extra)]
    _SCENES["position"] = (nd, params, base, more, extra, _oracle(O, mdl, nd, base), _oracle(O, mdl, nd, more))
    return _SCENES["position"]


def test_fill_by_list_position(engine, rsa, O):
    """fill[] is never cleared, and in a tick with hits it goes by list position.  Sequence 1 claims for every frame (positions
    are frames), sequence 2 serves every frame and writes nothing, sequence 3 adds nine never-seen sources at scattered places:
    their lists must be filled from THEIR frames, found through the list, past the stale words of sequence 1 -- sequence 4
    serves them against the oracle with nothing swept."""
    nd, params, base, more, extra, want_base, want_more = _position_scene(O)
    for s, x, w in zip(more, extra, want_more):
        at = np.searchsorted(s, np.sort(x))
        assert at.min() < 64 and at.max() >= 128 and len(np.unique(at // 64)) >= 3, at
        assert (_per_pkt(w, len(s))[at] > 0).all() and len(set(_per_pkt(w, len(s))[at].tolist())) > 1
    configure_engine(engine, nd, "logdist", params)
    _batch(engine, base, want_base, "sequence 1 (cold)")
    assert all(c > 0 for c in _swept(engine, 4))
    _batch(engine, base, want_base, "sequence 2 (all served)")
    assert _swept(engine, 4) == [0] * 4
    _batch(engine, more, want_more, "sequence 3 (new sources among served ones)")
    assert all(c > 0 for c in _swept(engine, 4))
    _batch(engine, more, want_more, "sequence 4 (all served)")
    assert _swept(engine, 4) == [0] * 4


# ---- 6. form switch ----------------------------------------------------------------------------------------------------------------

def _push(engine, nd, i):
    engine.update_node(int(i), nd.x[i], nd.y[i], nd.z[i], nd.txpower[i], int(nd.channel[i]), int(nd.enabled[i]), nd.rxprob[i], nd.txprob[i])


def _chained(engine, O, nd, mdl, srcs, state, what):
    """as _batch, with the oracle run here: the generator's state chains the ticks; -> its state after the sequence"""
    _run(engine, srcs)
    for b, s in enumerate(srcs):
        cpu = O.tick(mdl, nd, nd.packets(s, start_us=1000 * b, air_us=AIR), rng_state=state)
        state = cpu.rng_state
        assert_same(engine.batch_result_copy(b, len(s)), cpu, "%s, tick %d" % (what, b))
        assert engine.batch_result_count(b) == (cpu.count, 0)
    assert engine.rng_state == state, what
    return state


def test_form_switch(engine, rsa, O):
    """A stochastic batch (candidates form: fill[] by frame, hit[] tested per frame) between draw-free ones whose ticks mix known
    and new sources (heard form: fill[] by list position).  Every change of a node begins a new epoch, so each step runs cold
    and then mixed; every tick against the oracle, and the generator's state after every sequence."""
    nd = _layout(O, seed=151)
    params = dict(ld_sigma_db=4.0, ld_seed=11)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    ids = np.random.default_rng(152).permutation(N)
    known = [np.sort(ids[b * 170:(b + 1) * 170]).astype(np.int32) for b in range(4)]
    mixed = [_merge(k[::2], ids[1000 + b * 60:1000 + (b + 1) * 60]) for b, k in enumerate(known)]
    engine.profile_enable(1)
    engine.seed(21)
    state = O.lib().orc_jrandom_seed(21)

    def served():
        return sum(v[0] for k, v in engine.profile_kernels().items() if k.startswith("k_reorder_served_batch"))
    state = _chained(engine, O, nd, mdl, known, state, "draw-free, cold")
    state = _chained(engine, O, nd, mdl, mixed, state, "draw-free, mixed")
    assert all(c > 0 for c in _swept(engine, 4))
    n_served = served()
    assert n_served > 0
    lossy = np.random.default_rng(153).choice(N, 40, replace=False)
    nd.rxprob[lossy] = 0.6
    for i in lossy:
        _push(engine, nd, i)
    before = state
    state = _chained(engine, O, nd, mdl, known, state, "receivers that draw, cold")
    state = _chained(engine, O, nd, mdl, mixed, state, "receivers that draw, mixed")
    assert state != before and served() == n_served     # draws were consumed, in the candidates form
    nd.rxprob[lossy] = 1.0
    for i in lossy:
        _push(engine, nd, i)
    state = _chained(engine, O, nd, mdl, known, state, "draw-free again, cold")
    state = _chained(engine, O, nd, mdl, mixed, state, "draw-free again, mixed")
    assert all(c > 0 for c in _swept(engine, 4))
    state = _chained(engine, O, nd, mdl, mixed, state, "draw-free again, all served")
    assert _swept(engine, 4) == [0] * 4 and served() > n_served
