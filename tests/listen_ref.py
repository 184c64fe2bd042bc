"""Reference of the receiver listening schedules, on top of the untouched oracle: listening() in
Python integers straight from the spec (the 64-bit wrap included), apply() = a verdict column after E13 and the missed counts.
With the frame error model on it goes over errmodel_ref.Replay's verdicts.  The library's exports are never the source of an
expected value.  Also the schedules the GPU tests use over the scenes of errmodel_ref, so that the CPU tier can hold the
REFERENCE ALONE to the conditions that keep those tests from passing vacuously (tests/test_listen_ref.py)."""
import numpy as np

import errmodel_ref as R
from oracle import oracle as O

M64 = (1 << 64) - 1
DTYPE = np.dtype([("period_us", "<i8"), ("on_us", "<i8"), ("phase_us", "<i8")])
PERIODS = (0, 0, 1500, 2000, 3000, 7000, 125000)


def valid(s):
    period, on, phase = (int(v) for v in s)
    if period == 0:
        return on == 0 and phase == 0
    return period > 0 and 0 <= on <= period and 0 <= phase < period


def listening(s, t):
    """the rule: s = (period_us, on_us, phase_us), t an int64 time"""
    period, on, phase = (int(v) for v in s)
    if period == 0:
        return True
    d = (int(t) - phase) & M64          # uint64(t) - uint64(phase), wrapping
    if d >= 1 << 63:
        d -= 1 << 64                    # ... read as int64
    r = abs(d) % period                 # C's remainder truncates towards zero: the sign of d
    if d < 0:
        r = -r
    if r < 0:
        r += period
    return r < on


def table(sched):
    """any schedule table as a structured array"""
    a = np.asarray(sched)
    if a.dtype != DTYPE:
        a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1, 3).view(DTYPE).reshape(-1)
    return a


def apply(new_packets, res, sched, verdict=None):
    """the links of the oracle's TickResult `res` (res.pkt counts the positions of new_packets) under the schedules:
    -> (verdict column after E13, missed per node).  verdict: the column that is final under everything else (default
    res.verdict; errmodel_ref.Replay's .plain with the error model off)"""
    sched = table(sched)
    new_packets = np.atleast_1d(new_packets)
    before = np.asarray(res.verdict if verdict is None else verdict, dtype=np.uint8)
    after = before.copy()
    missed = np.zeros(len(sched), dtype=np.uint64)
    dst = np.asarray(res.dst, dtype=np.int64)
    for i in np.nonzero((before == O.DELIVERED) & (sched["period_us"][dst] != 0))[0]:
        j = int(dst[i])
        if not listening(sched[j], int(new_packets[int(res.pkt[i])]["start_us"])):
            after[i] = O.INTERFERED
            missed[j] += np.uint64(1)
    return after, missed


# ---- the schedules of tests/test_gpu_listen.py -----------------------------------------------------------------------------
# the edge cases a handful of reached receivers are forced to (the last two: a phase later than every frame start of the scenes,
# so d is negative -- one awake there, one asleep)
EDGES = {"on0": (2000, 0, 0), "full": (3000, 3000, 17), "p1_off": (1, 0, 0), "p1_on": (1, 1, 0),
         "neg_awake": (10_000_000, 5_000_000, 9_000_000), "neg_asleep": (10_000_000, 1000, 9_000_000)}


def schedule(n, seed, reached=()):
    """per node a period drawn from PERIODS, on_us uniform in 0 .. period, phase_us uniform in 0 .. period - 1; then the first
    len(EDGES) nodes of `reached` get the edge cases: -> (table, {edge name: node})"""
    rng = np.random.default_rng(seed)
    s = np.zeros(n, dtype=DTYPE)
    s["period_us"] = rng.choice(np.array(PERIODS, dtype=np.int64), n)
    s["on_us"] = rng.integers(0, s["period_us"] + 1)
    s["phase_us"] = rng.integers(0, np.maximum(s["period_us"], 1))
    edges = {}
    for (name, rec), node in zip(EDGES.items(), reached):
        s[int(node)] = rec
        edges[name] = int(node)
    assert all(valid(r) for r in s.tolist())
    return s, edges


def reached_receivers(pairs):
    """[(TickResult, verdict column)] -> the receivers with a delivered link, the most often delivered first (ties: lower index)"""
    cnt = {}
    for res, v in pairs:
        for j in np.asarray(res.dst)[np.asarray(v) == O.DELIVERED]:
            cnt[int(j)] = cnt.get(int(j), 0) + 1
    return [j for j, _ in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))]


def packets(nd, srcs, start, air):
    srcs = np.asarray(srcs, dtype=np.int32)
    new = nd.packets(np.where(srcs >= 0, srcs, 0), start, air)
    new["src"] = srcs
    return new


class Run:
    """a run of ticks on the SINR medium under a schedule: per tick the oracle's result (errmodel_ref.Replay), the verdict column
    before E13 (.before) and after it (.after); .missed the table after the run"""

    def __init__(self, nd, lists, starts, air, sched, em_seed=None):
        rep = R.Replay(nd, seed=R.SEED if em_seed is None else em_seed)
        self.res, self.before, self.after, self.new = [], [], [], []
        self.missed = np.zeros(nd.n, dtype=np.uint64)
        for l, s in zip(lists, starts):
            w, _ = rep.tick(s, l, s, air)
            new = packets(nd, l, s, air)
            before = w.plain if em_seed is None else w.verdict
            after, m = apply(new, w, sched, before)
            self.res.append(w)
            self.new.append(new)
            self.before.append(before)
            self.after.append(after)
            self.missed += m


def conditions(run, sched, edges):
    """what a scene has to show -> {flipped, kept_scheduled, kept_always, mixed, edges: {name: delivered-before links at it}}"""
    sched = table(sched)
    flipped = kept_s = kept_a = mixed = 0
    at_edge = {name: 0 for name in edges}
    for w, before, after in zip(run.res, run.before, run.after):
        was = before == O.DELIVERED
        fl = was & (after != O.DELIVERED)
        sch = sched["period_us"][np.asarray(w.dst, dtype=np.int64)] != 0
        flipped += int(fl.sum())
        kept_s += int((was & ~fl & sch).sum())
        kept_a += int((was & ~sch).sum())
        for q in np.unique(w.pkt[fl]):
            if ((w.pkt == q) & was & ~fl).any():
                mixed += 1
        for name, node in edges.items():
            at_edge[name] += int((was & (w.dst == node)).sum())
    return {"flipped": flipped, "kept_scheduled": kept_s, "kept_always": kept_a, "mixed": mixed, "edges": at_edge}


SCHED_SEED = 5
_SCENES = {}


def scene(name):
    """the scenes of errmodel_ref with their schedule, computed once and left unchanged:
    -> (nd, lists, starts, air, sched, edges, {em_seed or None: Run}); name: lone / serial / batch / batch_overlap"""
    if name not in _SCENES:
        extra = None
        if name == "lone":
            nd, srcs, start, air = R.scene_lone()
            lists, starts = [srcs], [start]
        elif name == "serial":
            nd, srcs, st, extra, air = R.scene_serial()
            lists, starts = [[int(q)] for q in srcs], [int(s) for s in st]
        else:
            nd, lists, starts, air = R.scene_batch(name == "batch_overlap")
        # the edge receivers are reached by delivered links with the error model on (so with it off as well)
        plain = Run(nd, lists, starts, air, np.zeros(nd.n, dtype=DTYPE), em_seed=R.SEED)
        sched, edges = schedule(nd.n, SCHED_SEED, reached_receivers(zip(plain.res, plain.before)))
        runs = {em: Run(nd, lists, starts, air, sched, em_seed=em) for em in (None, R.SEED)}
        _SCENES[name] = (nd, lists, starts, air, sched, edges, runs, extra)
    return _SCENES[name]
