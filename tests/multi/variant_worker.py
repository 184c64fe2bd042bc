"""One child of tests/test_gpu_variants.py: a FRESH process that runs the engine's scenarios under one or more settings of the
developer knobs (the RM_* environment variables that pick kernels, grids and code paths) and leaves the results in a directory
for the parent to compare with the oracle.  The parent never opens the GPU; this process never imports torch.

    python tests/multi/variant_worker.py <dir> <spec.json>

spec.json is a list of runs, {"name", "env", "scenarios", "proof"}: the run's knobs are put into os.environ (the knobs of the
run before that this one does not name are taken out again: only knobs read per call may share a process), then every scenario
runs on a new Engine.  A scenario named in "proof" runs once more with rm_profile_enable(1) on; the kernels it launched are
reported, and its links are compared with the oracle as well.  Written per run: <name>.npz (every tick's links) and <name>.json
(kernel names of the proof runs, the error of a scenario that raised).

The scenarios' inputs are seeded and built by the functions below, which the parent imports (no GPU there) to build the
oracle's side: expected(scenario, saved) -> {key: what the oracle says}.  The reception-stage scenarios compare against the
oracle's serial event replay in this process (the engine's and the oracle's steps interleave) and report a mismatch as the
scenario's error.
"""
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

AIR = 8128
FIELDS = ("pkt", "dst", "verdict", "rssi", "sinr", "pkt_interference")
SINR = {"ld_flags": 1, "ld_sigma_db": 4.0, "ld_seed": 77}
SHADOWED = {"ld_sigma_db": 4.0, "ld_seed": 9}


# ------------------------------------------------------------------------------------------------------ seeded inputs
def _nodes(O, n, seed, lossy=False, channels=False):
    from util import random_nodes
    rng = np.random.default_rng(seed + 1000)
    nd = random_nodes(O, n, 50.0 * np.sqrt(np.pi * n / 20.0), seed=seed)
    if lossy:
        nd.rxprob[rng.choice(n, n // 5, replace=False)] = 0.6
        nd.txprob[rng.choice(n, n // 50, replace=False)] = 0.5
    if channels:
        nd.channel[:] = 11 + rng.integers(0, 16, n)
    nd.enabled[rng.choice(n, max(1, n // 40), replace=False)] = 0     # disabled nodes: no frames heard, none sent
    nd.txprob[rng.choice(n, max(1, n // 100), replace=False)] = 0.0  # sources whose frames never leave
    return nd


def _sources(n, sizes, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, t, replace=False)).astype(np.int32) for t in sizes]


def inputs(O, name):
    """(nodes, model kind, model params, per-tick sources, tick length) of a scenario"""
    if name == "udgm_lone":      # UDGM, lossy links: java.util.Random draws; the last tick's links outnumber the pack's lanes
        return _nodes(O, 3001, 11, lossy=True), "udgm", dict(udgm_success_ratio_rx=0.8), _sources(3001, [120, 1, 64, 65, 2600], 12), 1000
    if name == "transmit":       # rm_transmit, one packet per call, draws
        return _nodes(O, 3001, 13, lossy=True), "udgm", dict(udgm_success_ratio_rx=0.9), _sources(3001, [1] * 12, 14), 1000
    if name == "logdist_batch":  # shadowed log-distance, one batch by source indices, ragged ticks
        return _nodes(O, 20011, 15), "logdist", dict(SHADOWED), _sources(20011, [1, 63, 64, 65, 257], 16), 1000
    if name == "big_batch":      # large enough for the near-frame lists and the grouped batch filter
        return _nodes(O, 70001, 17), "logdist", dict(SHADOWED), _sources(70001, [520, 530], 18), 1000
    if name == "sinr_lone":      # SINR, lone ticks, frames outlive their tick (8 ticks), 16 channels, a move before tick 3
        return _nodes(O, 6007, 19, channels=True), "logdist", dict(SINR), _sources(6007, [150, 1, 64, 150, 257, 90], 20), 1000
    if name == "sinr_batch":     # SINR, a batch of self-contained ticks (air time = tick length), 16 channels
        return _nodes(O, 6007, 21, channels=True), "logdist", dict(SINR), _sources(6007, [200, 1, 65, 300, 129], 22), 1000
    if name == "sinr_overlap":   # SINR, two batches whose frames outlive their ticks (rm_api_airbatch.cpp)
        return _nodes(O, 6007, 23, channels=True), "logdist", dict(SINR), _sources(6007, [120, 64, 1, 130, 65, 200], 24), 1000
    if name == "overflow":       # SINR, lone ticks; tick 3 does not fit the link capacity
        return _nodes(O, 6007, 25), "logdist", dict(SINR), _sources(6007, [10, 10, 10, 1800, 10, 10, 10], 26), 1000
    if name in ("gathered", "gathered_spatial"):   # a partitioned gathered batch, three ranks
        return _nodes(O, 9001, 27, channels=True), "logdist", dict(SHADOWED), _sources(9001, [240, 1, 241, 63], 28), 1000
    if name == "gathered_overlap":                  # the same with the SINR medium over two batches of overlapping ticks
        return _nodes(O, 9001, 29, channels=True), "logdist", dict(SINR), _sources(9001, [150, 64, 151, 100, 1, 120], 30), 1000
    raise KeyError(name)


SCENARIOS = ("udgm_lone", "transmit", "logdist_batch", "big_batch", "sinr_lone", "sinr_batch", "sinr_overlap", "overflow",
             "gathered", "gathered_spatial", "gathered_overlap", "events", "events_rings")
WORLD = 3
MOVE_TICK = 3       # sinr_lone: nodes 0..4 move 3 m before this tick
CAP_SMALL, CAP_LARGE = 1 << 16, 1 << 22   # (tick 3: ~75 k heard links; the others a few hundred)


# ------------------------------------------------------------------------------------------------------ GPU side
def _put(res, key, r):
    for f in FIELDS:
        res["%s.%s" % (key, f)] = np.asarray(getattr(r, f)).copy()
    res[key + ".count"] = np.array([r.count])
    res[key + ".pkt_offset"] = np.asarray(r.pkt_offset).astype(np.int64).copy()


def _engine(rsa, O, name):
    from util import configure_engine
    nd, kind, params, srcs, tlen = inputs(O, name)
    eng = rsa.Engine(0)
    configure_engine(eng, nd, kind, params)
    return eng, nd, srcs, tlen


def run_scenario(name, rsa, O, res, tag):
    from util import DeviceArray, to_tx_records
    if name == "events":
        return run_events(rsa, O)
    if name == "events_rings":
        return run_events_rings(rsa, O)
    keep = []
    if name.startswith("gathered"):
        return run_gathered(name, rsa, O, res, tag)
    eng, nd, srcs, tlen = _engine(rsa, O, name)
    try:
        if name == "udgm_lone":
            eng.seed(77)
            for b, s in enumerate(srcs):
                t0 = b * tlen
                eng.tick_begin(t0, t0 + tlen)
                eng.enqueue_records(to_tx_records(rsa, nd.packets(s, t0, AIR)))
                r = eng.tick_flush() if b % 2 == 0 else eng.tick_flush_view()   # copied / in the pinned host block
                _put(res, "%s.%d" % (tag, b), r)
                res["%s.%d.rng" % (tag, b)] = np.array([eng.rng_state], dtype=np.uint64)
        elif name == "transmit":
            eng.seed(5)
            for b, s in enumerate(srcs):
                r = eng.transmit(int(s[0]), start_us=b * tlen, hex_length=20)
                _put(res, "%s.%d" % (tag, b), r)
                res["%s.%d.rng" % (tag, b)] = np.array([eng.rng_state], dtype=np.uint64)
        elif name in ("logdist_batch", "big_batch", "sinr_batch"):
            dev = [DeviceArray(s) for s in srcs]
            keep += dev
            tb = [b * tlen for b in range(len(srcs))]
            air = tlen if name == "sinr_batch" else AIR
            eng.batch_run_sources_device(tb, [t + tlen for t in tb], [d.ptr.value for d in dev], [len(s) for s in srcs], tb,
                                         [air] * len(srcs))
            for b, s in enumerate(srcs):
                _put(res, "%s.%d" % (tag, b), eng.batch_result_copy(b, len(s)))
        elif name == "sinr_overlap":
            half = len(srcs) // 2
            for h in range(2):
                part = srcs[h * half:(h + 1) * half]
                dev = [DeviceArray(s) for s in part]
                keep += dev
                tb = [(h * half + b) * tlen for b in range(len(part))]
                eng.batch_run_sources_device(tb, [t + tlen for t in tb], [d.ptr.value for d in dev], [len(s) for s in part], tb,
                                             [AIR] * len(part))
                for b, s in enumerate(part):
                    _put(res, "%s.%d" % (tag, h * half + b), eng.batch_result_copy(b, len(s)))
        elif name == "sinr_lone":
            for b, s in enumerate(srcs):
                if b == MOVE_TICK:
                    eng.move_nodes(np.arange(5, dtype=np.int32), nd.x[:5] + 3.0, nd.y[:5])
                    nd.x[:5] += 3.0
                d = DeviceArray(s)
                keep.append(d)
                eng.tick_run_sources_device(b * tlen, (b + 1) * tlen, d.ptr.value, len(s), b * tlen, AIR)
                _put(res, "%s.%d" % (tag, b), eng.result_copy(len(s)))
        elif name == "overflow":
            eng.set_link_capacity(CAP_SMALL)
            for b, s in enumerate(srcs):
                t0 = b * tlen
                eng.tick_begin(t0, t0 + tlen)
                eng.enqueue_records(to_tx_records(rsa, nd.packets(s, t0, AIR)))
                try:
                    r = eng.tick_flush(cap=CAP_LARGE)
                except rsa.RadioMediumError as e:     # (the dropped tick: reported, its frames stay on the air)
                    if "rm_set_link_capacity" not in str(e):
                        raise
                    res["%s.%d.dropped" % (tag, b)] = np.array([1])
                    eng.set_link_capacity(CAP_LARGE)
                    continue
                res["%s.%d.dropped" % (tag, b)] = np.array([0])
                _put(res, "%s.%d" % (tag, b), r)
        else:
            raise KeyError(name)
        return eng
    finally:
        for d in keep:
            d.free()


def run_gathered(name, rsa, O, res, tag):
    """every rank's context in turn (one GPU), each handed the same gathered source indices [rank][tick][slot]"""
    from radio_sim_amd import dist as D
    from util import DeviceArray, configure_engine
    nd, kind, params, srcs, tlen = inputs(O, name)
    n = nd.n
    if name == "gathered":
        own = D.owners(n, WORLD)

        def put(eng, r):
            lo, hi = D.partition(n, r, WORLD)
            eng.set_partition(lo, hi - lo)
    else:
        probe = rsa.Engine(0)
        try:
            probe.upload_table(nd)
            own = D.owners(n, WORLD, probe)
        finally:
            probe.close()

        def put(eng, r):
            eng.set_partition_spatial(r, WORLD)
    slots = max(int((own[s] == r).sum()) for s in srcs for r in range(WORLD)) + 2
    packed = np.full((WORLD, len(srcs), slots), -1, dtype=np.int32)
    for b, s in enumerate(srcs):
        for r in range(WORLD):
            mine = s[own[s] == r]
            packed[r, b, :len(mine)] = mine
    res[tag + ".own"] = own
    res[tag + ".packed"] = packed
    overlap = name == "gathered_overlap"
    batches = [list(range(len(srcs)))] if not overlap else [list(range(len(srcs) // 2)), list(range(len(srcs) // 2, len(srcs)))]
    engines = []
    devs = []
    try:
        for r in range(WORLD):
            eng = rsa.Engine(0)
            engines.append(eng)
            configure_engine(eng, nd, kind, params)
            put(eng, r)
        for ticks in batches:
            dev = DeviceArray(np.ascontiguousarray(packed[:, ticks, :]).reshape(-1))
            devs.append(dev)
            t0 = np.array(ticks, dtype=np.int64) * tlen
            for r, eng in enumerate(engines):
                eng.batch_run_gathered_sources_device(t0, t0 + tlen, dev.ptr.value, WORLD, slots, t0, AIR)
                for k, b in enumerate(ticks):
                    _put(res, "%s.%d.r%d" % (tag, b, r), eng.batch_result_copy(k, WORLD * slots))
        return engines
    finally:
        for d in devs:
            d.free()


def run_events(rsa, O):
    """the reception stage: lone ticks, batches handed over with rm_events_process_batch, plain drains -- checked here against
    the oracle's serial replay (tests/test_gpu_events_batch.py's Session)"""
    from test_gpu_events_batch import Session, run_plan
    engines = []
    for args, kw, plan in (((1501, "udgm", dict(udgm_success_ratio_rx=0.8)), dict(tick_styles=(1000, 1000, 10, 3000)),
                            (7, "lone", 1, 64, "drain", "lone", 7, 3, "drain", 1)),
                           ((2501, "logdist", dict(ld_flags=1, ld_sigma_db=4.0, ld_seed=5)),
                            dict(per_tick=40, hex_lengths=(10, 64, 254, 254), sinr=True, draws=False), (7, "lone", 1, 16, "drain", 7, "lone"))):
        n, kind, params = args
        eng = rsa.Engine(0)
        engines.append(eng)
        s = Session(O, rsa, eng, 100 + n, kind, params, n=n, **kw)
        if run_plan(s, plan) <= 0:
            raise AssertionError("the reception stage delivered nothing")
    return engines


def run_events_rings(rsa, O):
    """the reception stage on rings of 64 packets and a few thousand links (tests/events_ring_ref.py's scenes): a session that
    wraps both rings several times, lone ticks and batches mixed, and one whose packet ring refuses ticks (named by source indices:
    the lone ticks whose append RM_EV_FUSE keeps for the drain's first launch, or not) -- against the oracle's
    replay and the host model of the rings, as tests/test_gpu_events_rings.py holds them under the defaults"""
    import events_ring_ref as R
    from test_gpu_events_batch import Session, run_plan
    engines = []
    for (seed, kind, params, kw), plan, conditions in (
            (R.WRAP["udgm_draws"], R.MIXED_PLAN, lambda rep: R.wrap_conditions(rep, "udgm_draws")),
            (R.OVERFLOW["packets_sources"], ("lone",) * R.OVERFLOW_TICKS, lambda rep: R.overflow_conditions(rep, "packets", "packets"))):
        eng = rsa.Engine(0)
        engines.append(eng)
        s = Session(O, rsa, eng, seed, kind, params, **kw)
        if run_plan(s, plan) <= 0:
            raise AssertionError("the reception stage delivered nothing")
        conditions(s.rings.report())
    return engines


def main():
    out_dir, spec_path = sys.argv[1], sys.argv[2]
    with open(spec_path) as f:
        runs = json.load(f)
    import radio_sim_amd as rsa
    from oracle import oracle as O
    O.lib()
    base = dict(os.environ)
    prev = {}
    for run in runs:
        for k in prev:   # the run before's knobs go back to what this process inherited
            if k in base:
                os.environ[k] = base[k]
            else:
                del os.environ[k]
        os.environ.update(run["env"])
        prev = run["env"]
        res, report = {}, {"kernels": {}, "errors": {}}
        for sc in run["scenarios"]:
            for profiled in ((False, True) if sc in run.get("proof", ()) else (False,)):
                tag = sc + (".prof" if profiled else "")
                engines = []
                try:
                    if profiled:
                        # every context this scenario makes is profiled: Engine is wrapped for the scenario's duration
                        made = []
                        orig = rsa.Engine.__init__

                        def init(self, *a, _orig=orig, _made=made, **k):
                            _orig(self, *a, **k)
                            self.profile_enable(1)
                            _made.append(self)
                        rsa.Engine.__init__ = init
                        try:
                            got = run_scenario(sc, rsa, O, res, tag)
                        finally:
                            rsa.Engine.__init__ = orig
                        names = set()
                        for e in made:
                            names.update(e.profile_kernels().keys())
                        report["kernels"][sc] = sorted(names)
                        engines = made
                    else:
                        got = run_scenario(sc, rsa, O, res, tag)
                        engines = got if isinstance(got, list) else [got]
                except Exception as e:  # noqa: BLE001  (a refusal or a mismatch of the in-process replay is the scenario's result)
                    report["errors"][tag] = "%s: %s\n%s" % (type(e).__name__, e, traceback.format_exc(limit=4))
                finally:
                    for e in engines:
                        try:
                            e.close()
                        except Exception:  # noqa: BLE001
                            pass
        np.savez(os.path.join(out_dir, run["name"] + ".tmp.npz"), **res)
        os.replace(os.path.join(out_dir, run["name"] + ".tmp.npz"), os.path.join(out_dir, run["name"] + ".npz"))
        with open(os.path.join(out_dir, run["name"] + ".json"), "w") as f:
            json.dump(report, f, indent=1)
        print("variant run %s: %d scenarios, %d errors" % (run["name"], len(run["scenarios"]), len(report["errors"])), flush=True)


# ------------------------------------------------------------------------------------------------------ oracle side
def _want(O, mdl, nd, pk, first_new=0, state=0):
    return O.tick(mdl, nd, pk, first_new=first_new, rng_state=state)


def expected(O, name, saved=None):
    """{tick key: oracle TickResult (and .rng / .dropped expectations)} of a scenario; `saved` holds what a child wrote of
    inputs that depend on the engine (a spatial partition's owners)"""
    from util import oracle_model
    nd, kind, params, srcs, tlen = inputs(O, name)
    mdl = oracle_model(O, kind, params)
    out = {}
    if name == "udgm_lone":
        state = O.lib().orc_jrandom_seed(77)
        for b, s in enumerate(srcs):
            w = _want(O, mdl, nd, nd.packets(s, b * tlen, AIR), state=state)
            state = w.rng_state
            out[str(b)] = w
    elif name == "transmit":
        state = O.lib().orc_jrandom_seed(5)
        for b, s in enumerate(srcs):
            w = _want(O, mdl, nd, nd.packets(s[:1], b * tlen, 640), state=state)
            state = w.rng_state
            out[str(b)] = w
    elif name in ("logdist_batch", "big_batch", "sinr_batch"):
        air = tlen if name == "sinr_batch" else AIR
        for b, s in enumerate(srcs):
            out[str(b)] = _want(O, mdl, nd, nd.packets(s, b * tlen, air))
    elif name in ("sinr_lone", "sinr_overlap", "overflow"):
        onair = np.zeros(0, dtype=O.PACKET_DTYPE)
        for b, s in enumerate(srcs):
            t0 = b * tlen
            if name == "sinr_lone" and b == MOVE_TICK:
                nd.x[:5] += 3.0
            onair = onair[onair["start_us"] + onair["air_us"] > t0]
            new = nd.packets(s, t0, AIR)
            out[str(b)] = _want(O, mdl, nd, np.concatenate([onair, new]), first_new=len(onair))
            onair = np.concatenate([onair, new])
    elif name.startswith("gathered"):
        packed = saved["packed"]
        onair = np.zeros(0, dtype=O.PACKET_DTYPE)
        for b in range(packed.shape[1]):
            order = packed[:, b, :].reshape(-1)
            real = np.nonzero(order >= 0)[0]
            new = nd.packets(order[real], b * tlen, AIR)
            if name == "gathered_overlap":
                onair = onair[onair["start_us"] + onair["air_us"] > b * tlen]
                w = _want(O, mdl, nd, np.concatenate([onair, new]), first_new=len(onair))
                onair = np.concatenate([onair, new])
            else:
                w = _want(O, mdl, nd, new)
            w.real = real
            out[str(b)] = w
    else:
        raise KeyError(name)
    return out


if __name__ == "__main__":
    main()
