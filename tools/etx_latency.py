"""Latency of the measured-route query (rm_etx.hip) at 100 k and 1 M nodes, K = 8, one root (node 0), both modes.
One MI355X, one process.

  band        a caller's table in device memory: row j holds j +- 1 .. +- 4, 40 frames heard per entry, delivered by the tests' rule
              (tests/etx_ref.py).  A DEEP graph: the tree is n / 4 links deep, so the rounds are n / 4 and more and the host loop
              (one launch, one 8-byte copy, one wait per round) is what is measured.
  field       the context's own E14 tables over BASELINE configs[2]'s field (log-distance with shadowing): neighbors(RM_NB_HEARS, 8)
              -> rm_linkstats_watch_device, then PASSES passes in which every node transmits once (1000 sources per tick), min_heard 2.
              A SHALLOW graph.
  per shape and mode: the device form's wall time, rounds and examined nodes (rm_etx_last_work), and -- in runs of their own -- the
              kernels' dispatch intervals (rm_profile_kernels) summed per query, and what is left of the wall time (the host loop)
  yardstick   the route that exists without the query, in the same process: the whole table copied to the host (rm_linkstats_read for
              the field, a device-to-host copy of both arrays for the band) plus rm_etx_from_tables (a host Dijkstra).  Its costs and
              parents are compared with the query's once, before anything is timed.

Medians of `reps` runs after two warm-up runs, with min and max (the 1 M band and the yardsticks: 3 runs after one).  Prints one JSON line.
Run on the GPU box:  python tools/etx_latency.py [reps]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import radio_sim_amd as rsa  # noqa: E402
from radio_sim_amd import workload as W  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import etx_ref as E  # noqa: E402
from util import DeviceArray  # noqa: E402

TICK = W.TICK_US
AIR = 640
PER_TICK, LINK_CAP, PASSES = 1000, 1 << 21, 3
K = 8
MODES = (("inbound", rsa.ETX_INBOUND), ("both", rsa.ETX_BOTH))


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def timed(fn, reps, warm=2):
    out = []
    for rep in range(reps + warm):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            out.append((time.perf_counter() - t0) * 1e6)
    return stats(out)


def kernels(eng, fn, reps):
    """the kernels' own dispatch intervals per call of fn -> {kernel: stats + launches}"""
    per, launches = {}, {}
    for rep in range(reps):
        eng.profile_enable(1)
        fn()
        for kname, v in eng.profile_kernels().items():
            if kname.startswith("k_etx_"):
                per.setdefault(kname, []).append(v[1] * 1e3)
                launches[kname] = int(v[0])
        eng.profile_enable(0)
    return {kname: dict(stats(v), launches=launches[kname]) for kname, v in per.items()}


def measure(eng, n, prm_kw, dev_tables, host_tables, reps, slow):
    """one table, both modes -> {mode: figures}; host_tables(): the yardstick's copy of the whole table to the host"""
    d_cost, d_par, d_slot, d_lc, d_chl = (DeviceArray(nbytes=8 * n), DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n),
                                          DeviceArray(nbytes=4 * n))
    d_root = DeviceArray(np.zeros(1, dtype=np.int32))
    out = {}
    try:
        for name, mode in MODES:
            prm = rsa.Engine.etx_params(mode=mode, **prm_kw)

            def query():
                return eng.etx_routes_device(prm, d_root.ptr.value, 1, d_cost.ptr.value, d_par.ptr.value, d_slot.ptr.value, d_lc.ptr.value,
                                             d_chl.ptr.value, dev_tables=dev_tables)

            def yardstick():
                return rsa.Engine.etx_from_tables(host_tables(), prm, [0], fields=("parent",))

            tot = query()
            got, ytot = yardstick()
            assert ytot == tot, (ytot, tot)
            assert (got["cost"] == DeviceArray.read(d_cost.ptr.value, np.uint64, n)).all()
            assert (got["parent"] == DeviceArray.read(d_par.ptr.value, np.int32, n)).all()
            rounds, examined = eng.etx_last_work()
            print("%d nodes: %s, %d rounds" % (n, name, rounds), file=sys.stderr, flush=True)
            lc = DeviceArray.read(d_lc.ptr.value, np.uint32, n)
            r, w = (3, 1) if slow else (reps, 2)
            o = {"reached": tot["reached"], "max_cost": tot["max_cost"], "rounds": rounds, "examined_per_node": examined / n,
                 "parents_over_128": int((lc > 128).sum()), "query": timed(query, r, w)}
            ks = kernels(eng, query, r)
            o["kernels"] = ks
            relax = sum(v["median_us"] for k, v in ks.items() if k.startswith("k_etx_relax"))
            rest = sum(v["median_us"] for k, v in ks.items() if not k.startswith("k_etx_relax"))
            o.update(relax_sum_us=relax, other_kernels_us=rest, host_loop_remainder_us=o["query"]["median_us"] - relax - rest)
            o["yardstick"] = timed(yardstick, 3, 1)
            out[name] = o
    finally:
        for d in (d_cost, d_par, d_slot, d_lc, d_chl, d_root):
            d.free()
    return out


def band(n, reps):
    peer, heard, delivered = E.band(n, K)
    st = E.stats(heard, delivered)
    eng = rsa.Engine(0)
    eng.upload_nodes(np.zeros(n), np.arange(n, dtype=np.float64))
    d_peer, d_stats = DeviceArray(peer), DeviceArray(st)
    try:
        def host_tables():
            return (DeviceArray.read(d_peer.ptr.value, np.int32, n * K).reshape(n, K),
                    DeviceArray.read(d_stats.ptr.value, rsa.LINK_STATS_DTYPE, n * K).reshape(n, K))

        return measure(eng, n, dict(min_heard=4, max_link_cost=2000), (d_peer.ptr.value, d_stats.ptr.value, K), host_tables, reps, slow=n > 200_000)
    finally:
        d_peer.free()
        d_stats.free()
        eng.close()


def field(n, reps):
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(LINK_CAP)
    d_all = DeviceArray(np.arange(n, dtype=np.int32))
    try:
        eng.linkstats_enable(K)
        stage = eng.linkstats_stage_device()
        eng.neighbors_device(rsa.NB_HEARS, K, stage)
        eng.linkstats_watch_device(stage)
        n_ticks, clock = n // PER_TICK, 0
        ptrs = [d_all.ptr.value + 4 * PER_TICK * b for b in range(n_ticks)]
        for _ in range(PASSES):
            for b0 in range(0, n_ticks, rsa.MAX_BATCH):
                nb = min(rsa.MAX_BATCH, n_ticks - b0)
                t0 = [clock + TICK * b for b in range(nb)]
                clock += TICK * nb
                eng.batch_run_sources_device(t0, [t + TICK for t in t0], ptrs[b0:b0 + nb], [PER_TICK] * nb, t0, [AIR] * nb)
        eng.sync()
        print("%d nodes: the field's tables are counted" % n, file=sys.stderr, flush=True)

        def host_tables():
            return (eng.linkstats_peers(), eng.linkstats_read()[0])

        table = eng.linkstats_read()
        out = measure(eng, n, dict(min_heard=2, max_link_cost=2048), None, host_tables, reps, slow=False)
        out["table"] = {"ticks_counted": table[1]["ticks_counted"], "entries_heard_at_least_2": int((table[0]["heard"] >= 2).sum()),
                        "entries_with_losses": int((table[0]["heard"] > table[0]["delivered"]).sum()), "bytes": int(n * K * 52)}
        return out
    finally:
        d_all.free()
        eng.close()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0]) if args else 10)
    out = {"unit": "us per query; kernels: summed dispatch intervals per query", "K": K, "roots": 1, "field_passes": PASSES, "shapes": []}
    for n in (100_000, 1_000_000):
        out["shapes"].append({"nodes": n, "band": band(n, reps), "field": field(n, reps)})
        print(json.dumps(out["shapes"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
