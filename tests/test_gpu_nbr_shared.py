"""The heard form's lists shared among a device's contexts: engines on an equal table and medium are attached
to ONE pool of lists, so a source that one engine has swept, ranked and filled is served to the others -- from other streams,
at any time.  Nothing of it may show in the results: every tick of every engine here is held to the oracle bit for bit, and the
sweep's candidate counts (rm_slot_stats: 0 = every frame of the tick was served) tell served from swept.
The shapes are test_gpu_nbr_heard.py's: 6000 nodes, 5 ticks of 150 sources."""
import numpy as np
import pytest

from util import configure_engine, oracle_model, random_nodes, assert_same, DeviceArray

pytestmark = pytest.mark.gpu

AIR = 8128
N = 6000

CASES = [
    ("udgm", {}),
    ("logdist", dict(ld_sigma_db=0.0)),
    ("logdist", dict(ld_sigma_db=4.0, ld_seed=11)),
]
IDS = ["udgm", "logdist-s0", "logdist-s4"]


def _layout(O, seed):
    return random_nodes(O, N, 50.0 * np.sqrt(np.pi * N / 20.0), seed=seed)


def _ticks(n_ticks, per_tick, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(N, per_tick, replace=False)).astype(np.int32) for _ in range(n_ticks)]


class Issued:
    """a batch in flight: its source lists stay on the device until the results have been read"""

    def __init__(self, engine, srcs):
        self.engine, self.srcs = engine, srcs
        self.dev = [DeviceArray(s) for s in srcs]
        self.starts = [1000 * b for b in range(len(srcs))]
        engine.batch_run_sources_device(self.starts, [s + 1000 for s in self.starts], [d.ptr.value for d in self.dev], [len(s) for s in srcs],
                                        self.starts, [AIR] * len(srcs))

    def check(self, want, what):
        """every tick against the oracle's; -> the sweep's candidates per tick"""
        try:
            for b, s in enumerate(self.srcs):
                assert_same(self.engine.batch_result_copy(b, len(s)), want[b], "%s, tick %d" % (what, b))
                assert self.engine.batch_result_count(b) == (want[b].count, 0)
            return [self.engine.slot_stats(b)[0] for b in range(len(self.srcs))]
        finally:
            for d in self.dev:
                d.free()
            self.dev = []


class Oracle:
    """the oracle's answer per tick, computed once per source list (no draw happens in these scenes: a tick's result depends on
    its sources alone)"""

    def __init__(self, O, nd, kind, params):
        self.O, self.nd, self.mdl, self.memo = O, nd, oracle_model(O, kind, params), {}

    def __call__(self, srcs):
        out = []
        for b, s in enumerate(srcs):
            key = (b, s.tobytes())
            if key not in self.memo:
                self.memo[key] = self.O.tick(self.mdl, self.nd, self.nd.packets(s, start_us=1000 * b, air_us=AIR))
            out.append(self.memo[key])
        return out


def _batch(engine, oracle, srcs, what):
    want = oracle(srcs)
    return Issued(engine, srcs).check(want, what), want


def _engines(rsa, count):
    return [rsa.Engine(0) for _ in range(count)]


def _close(engines):
    for e in engines:
        e.close()


@pytest.mark.parametrize("kind,params", CASES, ids=IDS)
def test_sharing(rsa, O, kind, params):
    """A runs a batch and is waited for; B, on the same table and medium, is served all of it from A's lists; a mixed batch on B
    sweeps the new sources only."""
    nd = _layout(O, seed=105)
    oracle = Oracle(O, nd, kind, params)
    srcs = _ticks(5, 150, seed=103)
    a, b = _engines(rsa, 2)
    try:
        configure_engine(a, nd, kind, params)
        configure_engine(b, nd, kind, params)
        first, want = _batch(a, oracle, srcs, "%s, A" % kind)
        assert all(w.count > 0 for w in want)
        assert all(c >= w.count for c, w in zip(first, want)), first            # A swept every frame
        a.sync()
        swept, _ = _batch(b, oracle, srcs, "%s, B served by A" % kind)
        assert swept == [0] * len(srcs), swept
        mixed = [np.unique(np.concatenate([s[::2], t])).astype(np.int32) for s, t in zip(srcs, _ticks(5, 90, seed=104))]
        swept, _ = _batch(b, oracle, mixed, "%s, B mixed" % kind)
        assert all(0 < c < f for c, f in zip(swept, first)), (swept, first)     # the new sources only
        b.sync()
        swept, _ = _batch(a, oracle, mixed, "%s, A served by B" % kind)
        assert swept == [0] * len(mixed), swept
    finally:
        _close([a, b])


@pytest.mark.parametrize("kind,params", CASES, ids=IDS)
def test_several_streams(rsa, O, kind, params):
    """Three engines, each on the stream its context owns (bench.py hands each context a stream of its own: the same
    arrangement), issue overlapping batches in turn with no wait between them: in every round each engine gets two batches back to
    back -- six launch sequences in flight over one pool, claiming, filling, publishing and serving each other's sources -- and the
    second one of each engine is held to the oracle.  The last round, issued after a wait, sweeps nothing anywhere."""
    nd = _layout(O, seed=115)
    oracle = Oracle(O, nd, kind, params)
    sets = [_ticks(5, 150, seed=120 + i) for i in range(4)]
    # (overlap inside a round as well: every set shares half of each tick's sources with the next one)
    sets = [[np.unique(np.concatenate([s, t[::2]])).astype(np.int32) for s, t in zip(sets[i], sets[(i + 1) % 4])] for i in range(4)]
    engines = _engines(rsa, 3)
    try:
        for e in engines:
            configure_engine(e, nd, kind, params)
        for rnd in range(3):
            warm = [Issued(e, sets[(rnd + j) % 4]) for j, e in enumerate(engines)]
            held = [Issued(e, sets[(rnd + j + 1) % 4]) for j, e in enumerate(engines)]
            for j, h in enumerate(held):
                h.check(oracle(h.srcs), "%s, round %d, engine %d" % (kind, rnd, j))
            for w in warm:
                for d in w.dev:
                    d.free()
        for e in engines:
            e.sync()
        last = [Issued(e, sets[j]) for j, e in enumerate(engines)]
        for j, h in enumerate(last):
            swept = h.check(oracle(h.srcs), "%s, last round, engine %d" % (kind, j))
            assert swept == [0] * len(h.srcs), (j, swept)
    finally:
        _close(engines)


@pytest.mark.parametrize("what", ["seed", "parameter", "node"])
def test_no_sharing_across_a_difference(rsa, O, what):
    """Another seed of the shadowing, another parameter of the medium, or one node moved before the first batch: B sweeps
    everything, and equals the oracle of what IT holds."""
    kind, params = "logdist", dict(ld_sigma_db=4.0, ld_seed=11)
    nd = _layout(O, seed=125)
    nd_b, params_b = nd, dict(params)
    if what == "seed":
        params_b["ld_seed"] = 12
    elif what == "parameter":
        params_b["ld_exponent"] = 3.1
    else:
        nd_b = _layout(O, seed=125)
        nd_b.x[17] += 3.0
    srcs = _ticks(5, 150, seed=126)
    a, b = _engines(rsa, 2)
    try:
        configure_engine(a, nd, kind, params)
        configure_engine(b, nd_b, kind, params_b)
        first, want = _batch(a, Oracle(O, nd, kind, params), srcs, "A")
        a.sync()
        swept, want_b = _batch(b, Oracle(O, nd_b, kind, params_b), srcs, "B, another " + what)
        assert all(w.count > 0 for w in want_b)
        assert all(c >= w.count for c, w in zip(swept, want_b)), swept
        swept, _ = _batch(a, Oracle(O, nd, kind, params), srcs, "A again")
        assert swept == [0] * len(srcs)
    finally:
        _close([a, b])


def _push(engine, nd, i):
    engine.update_node(int(i), nd.x[i], nd.y[i], nd.z[i], nd.txpower[i], int(nd.channel[i]), int(nd.enabled[i]), nd.rxprob[i], nd.txprob[i])


@pytest.mark.parametrize("kind,params", CASES, ids=IDS)
def test_detach(rsa, O, kind, params):
    """After sharing, B updates one node: it leaves the pool.  B's next batch is B's table's and sweeps; A's is the old table's and
    is served; B's second batch is served from its new pool."""
    nd = _layout(O, seed=135)
    nd_b = _layout(O, seed=135)
    srcs = _ticks(5, 150, seed=136)
    a, b = _engines(rsa, 2)
    try:
        configure_engine(a, nd, kind, params)
        configure_engine(b, nd, kind, params)
        old = Oracle(O, nd, kind, params)
        _batch(a, old, srcs, "A")
        a.sync()
        swept, _ = _batch(b, old, srcs, "B shares")
        assert swept == [0] * len(srcs)
        mover = int(srcs[0][3])
        nd_b.x[mover] += 20.0
        nd_b.y[mover] -= 10.0
        _push(b, nd_b, mover)
        new = Oracle(O, nd_b, kind, params)
        swept, want = _batch(b, new, srcs, "B, one node moved")
        assert all(c >= w.count > 0 for c, w in zip(swept, want)), swept      # every frame swept
        swept, _ = _batch(a, old, srcs, "A, the old table")
        assert swept == [0] * len(srcs), swept
        swept, _ = _batch(b, new, srcs, "B again")
        assert swept == [0] * len(srcs), swept
    finally:
        _close([a, b])


def test_lifetime(rsa, O):
    """A is closed while B goes on: B is still served and correct.  When every engine is closed nothing is remembered: a new
    engine on the same table sweeps everything."""
    kind, params = "logdist", dict(ld_sigma_db=4.0, ld_seed=11)
    nd = _layout(O, seed=145)
    oracle = Oracle(O, nd, kind, params)
    srcs = _ticks(5, 150, seed=146)
    a, b = _engines(rsa, 2)
    try:
        configure_engine(a, nd, kind, params)
        configure_engine(b, nd, kind, params)
        first, want = _batch(a, oracle, srcs, "A")
        a.sync()
        assert _batch(b, oracle, srcs[:2], "B, two ticks")[0] == [0, 0]
        a.close()
        assert _batch(b, oracle, srcs, "B, A closed")[0] == [0] * len(srcs)
        more = _ticks(5, 150, seed=147)
        swept, _ = _batch(b, oracle, more, "B, new sources")
        assert all(c > 0 for c in swept)
        assert _batch(b, oracle, more, "B, new sources again")[0] == [0] * len(more)
    finally:
        _close([a, b])
    c = rsa.Engine(0)
    try:
        configure_engine(c, nd, kind, params)
        swept, _ = _batch(c, oracle, srcs, "a new engine")
        assert all(s >= w.count > 0 for s, w in zip(swept, want)), (swept, first)
    finally:
        c.close()


def test_empty_lists_are_shared(rsa, O):
    """Sources that reach nobody: a tick of nothing else still publishes their zero-length lists, and the other engine is served
    them as such -- the sweep's candidates of that tick, which A had, are gone on B."""
    kind, params = "logdist", dict(ld_sigma_db=4.0, ld_seed=11)
    nd = _layout(O, seed=155)
    pick = _ticks(1, 900, seed=156)[0]
    nd.txpower[pick] = -22.0
    mdl = oracle_model(O, kind, params)
    per = np.bincount(O.tick(mdl, nd, nd.packets(pick, start_us=0, air_us=AIR)).pkt, minlength=len(pick))
    silent, heard = pick[per == 0], pick[per > 0]
    assert len(silent) >= 150 and len(heard) >= 75, (len(silent), len(heard))
    srcs = [silent[:150], np.sort(np.concatenate([silent[75:150], heard[:75]])).astype(np.int32), heard[:150]]
    oracle = Oracle(O, nd, kind, params)
    a, b = _engines(rsa, 2)
    try:
        configure_engine(a, nd, kind, params)
        configure_engine(b, nd, kind, params)
        first, want = _batch(a, oracle, srcs, "A")
        assert want[0].count == 0 and first[0] > 0, first        # nobody hears them, yet the sweep had candidates to evaluate
        a.sync()
        swept, _ = _batch(b, oracle, srcs, "B")
        assert swept == [0, 0, 0], swept
    finally:
        _close([a, b])


def test_a_dropped_tick_publishes_nothing(rsa, O):
    """A's link capacity is below one tick's heard total: the tick is dropped, and none of its sources gets a list -- B, with room,
    sweeps exactly that tick's new sources and is served the rest."""
    kind, params = "logdist", dict(ld_sigma_db=0.0)
    nd = _layout(O, seed=165)
    small = _ticks(4, 150, seed=166)
    loud = np.setdiff1d(_ticks(1, 260, seed=167)[0], np.concatenate(small))[:200].astype(np.int32)
    nd.txpower[np.concatenate(small)] = -14.0
    nd.txpower[loud] = 10.0
    srcs = [small[0], small[1], loud, small[2], small[3]]
    oracle = Oracle(O, nd, kind, params)
    want = oracle(srcs)
    cap = 1 << 14
    assert 20 * max(w.count for b, w in enumerate(want) if b != 2) < cap < want[2].count
    a, b = _engines(rsa, 2)
    try:
        configure_engine(a, nd, kind, params)
        configure_engine(b, nd, kind, params)
        a.set_link_capacity(cap)
        run = Issued(a, srcs)
        try:
            for t, s in enumerate(srcs):
                cnt, dropped = a.batch_result_count(t)
                assert dropped == (1 if t == 2 else 0), t
                if t != 2:
                    assert_same(a.batch_result_copy(t, len(s)), want[t], "A, tick %d" % t)
        finally:
            for d in run.dev:
                d.free()
        a.sync()
        swept, _ = _batch(b, oracle, srcs, "B")
        assert swept[2] > 0 and all(c == 0 for t, c in enumerate(swept) if t != 2), swept
        b.sync()
        a.set_link_capacity(1 << 20)
        swept, _ = _batch(a, oracle, srcs, "A, with room")
        assert swept == [0] * len(srcs), swept
    finally:
        _close([a, b])
