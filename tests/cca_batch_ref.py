"""Expected values of a carrier-sense gated BATCH from the oracle alone.  tests/cca_ref.py::Chain.gated_tick
called tick by tick IS E7's definition; this module only adds the scene with the hand-built chain of nodes, the cached run of a scene
through that chain, and the two wrong readings of E7 that the tests hold the scenes against.  No engine code is involved."""
import itertools

import numpy as np

import cca_ref as CR
import energy_ref as R

_CACHE = {}


class ChainScene:
    """Scene "multi" (unchanged) plus three nodes A, B, C on a line far outside its square, spaced so that -- under the scene's
    shadowing seed -- B senses A, C senses B, and C does not sense A.  Ticks 0 .. 3 of the scene carry them as extra candidates:
    A in tick 0, B in tick 1, C and B in tick 2, A in tick 3."""

    def __init__(self, O):
        base = CR.Scene(O, "multi")
        self.name, self.params, self.threshold = "chain", base.params, base.threshold
        self.sample_at, self.start_at, self.n_ticks = base.sample_at, base.start_at, 4
        n = base.nd.n
        nd = O.NodeTable(n + 3)
        nd.x[:n], nd.y[:n] = base.nd.x, base.nd.y
        far = float(base.nd.x.max()) + 4000.0
        mdl = O.model(O.MODEL_LOGDIST, **self.params)
        one = lambda v: np.array([v], dtype=np.int32)
        busy = lambda frames, node: bool(R.channel_energy(O, mdl, nd, frames, 1, nodes=one(node), threshold=self.threshold)[1][0] & R.ED_BUSY)
        self.spacing = None
        # the links' shadowing is a hash of the two node indices: which of the three new nodes plays A, B and C, and the spacing, are
        # the first choice under which the three links are as the chain needs them
        for a, b, c in itertools.permutations((n, n + 1, n + 2)):
            for d in range(10, 200, 5):
                nd.x[[a, b, c]], nd.y[[a, b, c]] = [far, far + d, far + 2 * d], far
                fa, fb = nd.packets(one(a), 0, CR.AIR), nd.packets(one(b), 0, CR.AIR)
                if busy(fa, b) and not busy(fa, c) and busy(np.concatenate([fa, fb]), c):
                    self.spacing, self.a, self.b, self.c = d, a, b, c
                    break
            if self.spacing is not None:
                break
        assert self.spacing is not None, "no spacing puts B in A's range, C in B's and not in A's"
        self.nd = nd
        extra = ([self.a], [self.b], [self.c, self.b], [self.a])
        self.ticks = [np.concatenate([base.ticks[k], np.array(extra[k], dtype=np.int32)]) for k in range(4)]

    times = CR.Scene.times
    model = CR.Scene.model


def scene(O, name):
    key = ("scene", name)
    if key not in _CACHE:
        _CACHE[key] = ChainScene(O) if name == "chain" else CR.Scene(O, name)
    return _CACHE[key]


class Run:
    """a scene's first `ticks` ticks through the oracle chain, computed once and left unchanged: per tick flags, energy, Expected and
    the frames on the air after it"""

    def __init__(self, O, sc, ticks, threshold=None, lists=None):
        chain = CR.Chain(O, sc.nd, sc.model(O))
        self.flags, self.energy, self.exp, self.onair = [], [], [], []
        lists = sc.ticks[:ticks] if lists is None else lists
        self.lists = [np.asarray(s, dtype=np.int32) for s in lists]
        thr = sc.threshold if threshold is None else threshold
        for k, src in enumerate(self.lists):
            t0, tc, ts = sc.times(k)
            f, e, x = chain.gated_tick(t0, src, ts, CR.AIR, tc, thr)
            self.flags.append(f)
            self.energy.append(e)
            self.exp.append(x)
            self.onair.append(chain.onair.copy())


def run(O, name, ticks):
    key = ("run", name, ticks)
    if key not in _CACHE:
        _CACHE[key] = Run(O, scene(O, name), ticks)
    return _CACHE[key]


def wrong_readings(O, sc, r, first, last):
    """For the batch of ticks first .. last-1 of run `r`: the flags under two wrong readings of E7 -- "every earlier candidate of the
    batch is on the air" and "only the window counts, the earlier ticks of the batch do not" -> (all_kept, window_only), per tick."""
    mdl = sc.model(O)
    window = r.onair[first - 1] if first > 0 else np.zeros(0, dtype=O.PACKET_DTYPE)
    assumed = window
    all_kept, window_only = [], []
    for k in range(first, last):
        _, tc, ts = sc.times(k)
        src = r.lists[k]
        ok = np.flatnonzero((src >= 0) & (src < sc.nd.n))
        for frames, out in ((assumed, all_kept), (window, window_only)):
            f = np.zeros(len(src), dtype=np.uint8)
            if len(ok):
                f[ok] = R.channel_energy(O, mdl, sc.nd, frames, tc, nodes=src[ok], threshold=sc.threshold)[1]
            out.append(f)
        assumed = np.concatenate([assumed, sc.nd.packets(src[ok], ts, CR.AIR)])
    return all_kept, window_only
