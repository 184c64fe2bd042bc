"""The source candidate cache of the batched sweep: a context keeps, per source node, the receivers the sweep
found for it, and a later batch copies that list instead of sweeping the frame again.  Nothing of it may show in the results:
every tick of every batch here is held to the oracle bit for bit (heard set, order, rssi, verdict) -- with the lists being
filled, with every frame served from them, and after each kind of change that makes them stale."""
import numpy as np
import pytest

from util import configure_engine, oracle_model, random_nodes, assert_same, DeviceArray

pytestmark = pytest.mark.gpu

AIR = 8128
NC_KERNELS = ("k_nc_claim_batch", "k_nc_fill_batch", "k_nc_expand_batch")


@pytest.fixture(autouse=True, params=[None, "2"], ids=["", "near-lists"])
def near_lists(request, monkeypatch):
    """Every case twice: the filter the sizes here choose (256 shards per tick), and the 1024-receiver workgroups with the
    near-frame lists that the bench shape takes (64 shards per tick)."""
    if request.param:
        monkeypatch.setenv("RM_NEAR_LISTS", request.param)
        monkeypatch.setenv("RM_WG_RPT", "4")


def _layout(O, n, seed, side=None):
    return random_nodes(O, n, side if side else 50.0 * np.sqrt(np.pi * n / 20.0), seed=seed)


def _batch(engine, O, nd, mdl, srcs, state, what):
    """one launch sequence over the ticks `srcs`; every tick against the oracle; -> (generator state, oracle results)"""
    dev = [DeviceArray(s) for s in srcs]
    starts = [1000 * b for b in range(len(srcs))]
    engine.batch_run_sources_device(starts, [s + 1000 for s in starts], [d.ptr.value for d in dev], [len(s) for s in srcs], starts,
                                    [AIR] * len(srcs))
    want = []
    for b, s in enumerate(srcs):
        cpu = O.tick(mdl, nd, nd.packets(s, start_us=starts[b], air_us=AIR), rng_state=state)
        state = cpu.rng_state
        assert_same(engine.batch_result_copy(b, len(s)), cpu, "%s, tick %d" % (what, b))
        assert engine.batch_result_count(b) == (cpu.count, 0)
        want.append(cpu)
    assert engine.rng_state == state
    for d in dev:
        d.free()
    return state, want


def _ticks(n, n_ticks, per_tick, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, per_tick, replace=False)).astype(np.int32) for _ in range(n_ticks)]


def _push(engine, nd, i):
    engine.update_node(int(i), nd.x[i], nd.y[i], nd.z[i], nd.txpower[i], int(nd.channel[i]), int(nd.enabled[i]), nd.rxprob[i], nd.txprob[i])


def _heard_by(res, pkt):
    return set(res.dst[res.pkt == pkt].tolist())


CASES = [
    ("udgm", {}, False),
    ("udgm", dict(udgm_success_ratio_rx=0.8), True),        # every heard link draws: the shared generator chains ticks and batches
    ("udgm_const", {}, False),
    ("logdist", dict(ld_sigma_db=0.0), False),
    ("logdist", dict(ld_sigma_db=4.0, ld_seed=11), False),  # the shadowing table decides what a list holds
]


@pytest.mark.parametrize("kind,params,lossy", CASES)
def test_the_same_sources_in_consecutive_batches(engine, rsa, O, kind, params, lossy):
    n = 6000
    nd = _layout(O, n, seed=5)
    if lossy:
        rng = np.random.default_rng(105)
        nd.rxprob[rng.choice(n, n // 5, replace=False)] = 0.6
        nd.txprob[rng.choice(n, n // 50, replace=False)] = 0.5
        nd.enabled[rng.choice(n, n // 40, replace=False)] = 0
    configure_engine(engine, nd, kind, params)
    engine.profile_enable(1)
    engine.seed(77)
    state = O.lib().orc_jrandom_seed(77)
    mdl = oracle_model(O, kind, params)
    srcs = _ticks(n, 5, 150, seed=3)
    for rep in range(3):    # the lists are filled, then every frame is served from them, twice
        state, want = _batch(engine, O, nd, mdl, srcs, state, "%s, batch %d" % (kind, rep))
        assert sum(w.count for w in want) > 0
    # other sources over the same table: a mix of served and swept frames in every tick
    mixed = [np.unique(np.concatenate([s[::2], t])).astype(np.int32) for s, t in zip(srcs, _ticks(n, 5, 90, seed=4))]
    state, _ = _batch(engine, O, nd, mdl, mixed, state, "%s, mixed batch" % kind)
    ran = engine.profile_kernels()
    for k in NC_KERNELS:
        assert any(name.startswith(k) for name in ran), (k, sorted(ran))


def test_a_source_twice_inside_one_batch(engine, rsa, O):
    n = 6000
    nd = _layout(O, n, seed=6)
    params = dict(ld_sigma_db=4.0, ld_seed=3)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    a, b = _ticks(n, 2, 200, seed=8)
    both = np.unique(np.concatenate([a[:100], b[:100]])).astype(np.int32)
    srcs = [a, both, a, b, both]            # every source of tick 0 again in tick 2, half of it in ticks 1 and 4
    engine.seed(21)
    state = O.lib().orc_jrandom_seed(21)
    for rep in range(2):
        state, _ = _batch(engine, O, nd, mdl, srcs, state, "batch %d" % rep)
    _batch(engine, O, nd, mdl, [b, a], state, "the same sources, other ticks")


def test_every_invalidation_is_seen_by_the_next_batch(engine, rsa, O):
    n = 6000
    nd = _layout(O, n, seed=7)
    params = dict(ld_sigma_db=4.0, ld_seed=11)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    srcs = _ticks(n, 4, 160, seed=9)
    s0, s1 = int(srcs[0][0]), int(srcs[1][5])
    engine.seed(21)
    state = O.lib().orc_jrandom_seed(21)

    def twice(what):    # the batch that has to see the change (its lists are filled again), then one served from the new lists
        nonlocal state
        state, first = _batch(engine, O, nd, mdl, srcs, state, what)
        state, _ = _batch(engine, O, nd, mdl, srcs, state, what + ", again")
        return first

    twice("before any change")
    # a receiver moved into a cached source's reach, and out of it again
    d = np.hypot(nd.x - nd.x[s0], nd.y - nd.y[s0])
    r = int(np.argmax(d))
    assert r not in _heard_by(twice("unchanged")[0], 0)
    home = (nd.x[r], nd.y[r])
    nd.x[r], nd.y[r] = nd.x[s0] + 1.0, nd.y[s0]
    _push(engine, nd, r)
    assert r in _heard_by(twice("a receiver moved into reach")[0], 0)
    nd.x[r], nd.y[r] = home
    engine.move_nodes([r], [home[0]], [home[1]])
    assert r not in _heard_by(twice("... and out of it")[0], 0)
    # the source's tx power and channel
    before = _heard_by(twice("unchanged")[0], 0)
    nd.txpower[s0] = -15.0
    _push(engine, nd, s0)
    less = _heard_by(twice("tx power lowered")[0], 0)
    assert less < before
    nd.txpower[s0] = 6.0
    _push(engine, nd, s0)
    assert _heard_by(twice("tx power raised")[0], 0) > before
    nd.channel[s0] = 5
    _push(engine, nd, s0)
    assert not _heard_by(twice("the source on another channel")[0], 0)
    # a radio switched off
    k1 = int(np.nonzero(srcs[1] == s1)[0][0])
    heard = sorted(_heard_by(twice("unchanged")[1], k1))
    assert heard
    off = heard[0]
    nd.enabled[off] = 0
    _push(engine, nd, off)
    assert off not in _heard_by(twice("a radio switched off")[1], k1)
    # the seed of the shadowing, then the model
    params = dict(ld_sigma_db=4.0, ld_seed=12)
    engine.set_model(rsa.MODEL_LOGDIST, ld_sigma_db=4.0, ld_seed=12)
    mdl = oracle_model(O, "logdist", params)
    twice("another shadowing seed")
    engine.set_model(rsa.MODEL_UDGM)
    mdl = oracle_model(O, "udgm", {})
    twice("another medium")
    engine.set_model(rsa.MODEL_LOGDIST, ld_sigma_db=4.0, ld_seed=12)
    mdl = oracle_model(O, "logdist", params)
    twice("the first medium again")
    # enough moves for a new sort of the engine order: the lists hold engine positions
    builds = engine.receiver_table_builds()
    rng = np.random.default_rng(10)
    movers = rng.choice(n, n // 3, replace=False).astype(np.int32)
    side = 50.0 * np.sqrt(np.pi * n / 20.0)
    nd.x[movers] = rng.uniform(0, side, len(movers))
    nd.y[movers] = rng.uniform(0, side, len(movers))
    engine.move_nodes(movers, nd.x[movers], nd.y[movers])
    twice("a third of the nodes moved")
    assert engine.receiver_table_builds() > builds
    # a new table
    nd2 = _layout(O, n, seed=70)
    engine.upload_table(nd2)
    nd = nd2
    twice("a new table")


def test_an_arena_too_small_for_all_sources(engine, rsa, O):
    """96 arena entries per node; here a source has some 300 candidates (at most the list cap of 1024): a fifth of the sources
    get a list, the others are swept every time."""
    n = 2000
    nd = _layout(O, n, seed=12, side=270.0)
    params = dict(ld_sigma_db=0.0)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    perm = np.random.default_rng(13).permutation(n)
    srcs = [np.sort(perm[i * 250:(i + 1) * 250]).astype(np.int32) for i in range(8)]    # every node transmits
    engine.seed(21)
    state = O.lib().orc_jrandom_seed(21)
    for rep in range(3):
        state, want = _batch(engine, O, nd, mdl, srcs, state, "batch %d" % rep)
    assert sum(w.count for w in want) > 96 * n


def test_a_source_over_the_list_cap(engine, rsa, O):
    """Strong sources with some 1900 candidates (over the cap of 1024: never cached) among weak ones with a handful."""
    n = 3000
    nd = _layout(O, n, seed=14, side=150.0)
    rng = np.random.default_rng(15)
    weak = rng.choice(n, n // 2, replace=False)
    nd.txpower[weak] = -30.0
    params = dict(ld_sigma_db=2.0, ld_seed=5)
    configure_engine(engine, nd, "logdist", params)
    mdl = oracle_model(O, "logdist", params)
    srcs = _ticks(n, 4, 40, seed=16)
    engine.seed(21)
    state = O.lib().orc_jrandom_seed(21)
    for rep in range(3):
        state, want = _batch(engine, O, nd, mdl, srcs, state, "batch %d" % rep)
    per_pkt = np.concatenate([np.bincount(w.pkt, minlength=40) for w in want])
    assert per_pkt.max() > 1024 and (per_pkt < 100).sum() > 20
