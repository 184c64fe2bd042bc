"""Latency of the route query (rm_routes.hip) at the bench's 100 k and 1 M node shapes (the log-distance medium with
shadowing, BASELINE configs[2]'s field), one root (node 0), both directions.  One process.

  none                RM_EM_NONE at the model's defaults, beside rm_hops_query_device on the same context: the same answer (compared
                      once, before anything is timed), claiming instead of relaxing -- the floor
  marginal            RM_EM_OQPSK_250K, 4064 us frames, 4 us per bit, cap 1024, min_rssi -inf, with ld_sensitivity_dbm = -103: rounds,
                      the frontier entries over all rounds as a multiple of the node count (rm_routes_last_work), the query's wall
                      time, and -- in runs of their own -- the kernels' dispatch intervals (rm_profile_kernels) summed per query:
                      the relaxation launches, the parent pass, and what is left of the wall time (the host loop: one 4-byte copy and
                      one wait per round)
  yardstick           (100 k nodes only, RM_NB_HEARD_BY) the route that exists without the query: every node as a source through
                      rm_batch_run_sources_device, the heard links taken from the host results, then rm_routes_from_links (a host
                      Dijkstra).  Its costs and parents are compared with the query's once, before anything is timed.

Medians of `reps` runs after two warm-up runs, with min and max.  Prints one JSON line.
Run on the GPU box:  python tools/routes_latency.py [reps]
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
from util import DeviceArray  # noqa: E402

TICK = W.TICK_US
AIR = 640
PER_TICK, LINK_CAP = 1000, 1 << 21
SENS_MARGINAL = -103.0
NOISE_DBM = -100.0   # the model's default noise floor
CLOCK = [0]   # every batch takes the next ticks in time


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


def kernels(eng, fn, reps, prefixes):
    """the kernels' own dispatch intervals per call of fn -> {kernel: stats + launches}"""
    per, launches = {}, {}
    for rep in range(reps):
        eng.profile_enable(1)
        fn()
        for kname, v in eng.profile_kernels().items():
            if kname.startswith(prefixes):
                per.setdefault(kname, []).append(v[1] * 1e3)
                launches[kname] = int(v[0])
        eng.profile_enable(0)
    return {kname: dict(stats(v), launches=launches[kname]) for kname, v in per.items()}


def yardstick(eng, n, ptrs, params):
    """all HEARD_BY links through the evaluating path, then the host Dijkstra -> (outputs, totals, links)"""
    node, far, rssi = [], [], []
    n_ticks = n // PER_TICK
    for b0 in range(0, n_ticks, rsa.MAX_BATCH):
        nb = min(rsa.MAX_BATCH, n_ticks - b0)
        t0 = [CLOCK[0] + TICK * b for b in range(nb)]
        CLOCK[0] += TICK * nb
        eng.batch_run_sources_device(t0, [t + TICK for t in t0], ptrs[b0:b0 + nb], [PER_TICK] * nb, t0, [AIR] * nb)
        res, _ = eng.batch_result_view(nb)
        for b, r in enumerate(res):
            assert r.count < LINK_CAP
            off = np.asarray(r.pkt_offset, dtype=np.int64)
            node.append(np.repeat(np.arange(PER_TICK, dtype=np.int32) + (b0 + b) * PER_TICK, np.diff(off)))
            far.append(np.array(r.dst[:r.count], dtype=np.int32))
            rssi.append(np.array(r.rssi[:r.count], dtype=np.float64))
    node, far, rssi = np.concatenate(node), np.concatenate(far), np.concatenate(rssi)
    out, tot = rsa.Engine.routes_from_links(n, node, far, rssi, params, NOISE_DBM, [0], fields=("parent",))
    return out, tot, len(node)


def shape(n, reps, with_yardstick):
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(LINK_CAP)
    d_cost, d_par, d_rssi, d_lc, d_chl = (DeviceArray(nbytes=8 * n), DeviceArray(nbytes=4 * n), DeviceArray(nbytes=8 * n), DeviceArray(nbytes=4 * n),
                                          DeviceArray(nbytes=4 * n))
    d_hop, d_hpar = DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n)
    d_root = DeviceArray(np.zeros(1, dtype=np.int32))
    keep = [d_cost, d_par, d_rssi, d_lc, d_chl, d_hop, d_hpar, d_root]
    out = {"nodes": n, "roots": 1}
    try:
        def routes(params):
            return eng.routes_device(params, d_root.ptr.value, 1, d_cost.ptr.value, d_par.ptr.value, d_rssi.ptr.value, d_lc.ptr.value, d_chl.ptr.value)

        def hops(direction):
            return eng.hops_device(direction, d_root.ptr.value, 1, d_hop.ptr.value, d_hpar.ptr.value, d_rssi.ptr.value, d_chl.ptr.value)

        dirs = (("heard_by", rsa.NB_HEARD_BY), ("hears", rsa.NB_HEARS))
        # (a) RM_EM_NONE beside the hop query, at the model's defaults
        out["none"] = {}
        for name, d in dirs:
            prm = rsa.Engine.routes_params(d, kind=rsa.EM_NONE)
            ht, rt_ = hops(d), routes(prm)
            hop = DeviceArray.read(d_hop.ptr.value, np.int32, n).astype(np.int64)
            cost = DeviceArray.read(d_cost.ptr.value, np.uint64, n)
            assert (cost == np.where(hop >= 0, 128 * hop, -1).astype(np.uint64)).all()
            assert (DeviceArray.read(d_par.ptr.value, np.int32, n) == DeviceArray.read(d_hpar.ptr.value, np.int32, n)).all()
            rounds, entries = eng.routes_last_work()
            print("%d nodes: none, %s" % (n, name), file=sys.stderr, flush=True)
            out["none"][name] = {"reached": rt_["reached"], "max_hop": ht["max_hop"], "rounds": rounds, "entries_per_node": entries / n,
                                 "routes_query": timed(lambda: routes(prm), reps), "hops_query": timed(lambda: hops(d), reps),
                                 "kernels": kernels(eng, lambda: routes(prm), reps, ("k_route_", "k_nb_"))}
        # (b) the marginal links
        eng.set_model(rsa.MODEL_LOGDIST, **dict(kw, ld_sensitivity_dbm=SENS_MARGINAL))
        out["marginal"] = {}
        for name, d in dirs:
            print("%d nodes: marginal, %s" % (n, name), file=sys.stderr, flush=True)
            prm = rsa.Engine.routes_params(d)
            tot = routes(prm)
            rounds, entries = eng.routes_last_work()
            lc = DeviceArray.read(d_lc.ptr.value, np.uint32, n)
            o = {"reached": tot["reached"], "max_cost": tot["max_cost"], "rounds": rounds, "entries_per_node": entries / n,
                 "parents_over_128": int((lc > 128).sum()), "hops_max_hop": hops(d)["max_hop"], "query": timed(lambda: routes(prm), reps)}
            ks = kernels(eng, lambda: routes(prm), reps, ("k_route_", "k_nb_"))
            o["kernels"] = ks
            relax = sum(v["median_us"] for k, v in ks.items() if k.startswith("k_route_relax"))
            parent = sum(v["median_us"] for k, v in ks.items() if k.startswith("k_route_parent"))
            rest = sum(v["median_us"] for k, v in ks.items() if not k.startswith(("k_route_relax", "k_route_parent")))
            o.update(relax_sum_us=relax, parent_us=parent, other_kernels_us=rest, host_loop_remainder_us=o["query"]["median_us"] - relax - parent - rest)
            out["marginal"][name] = o
        # (c) the yardstick
        if with_yardstick:
            prm = rsa.Engine.routes_params(rsa.NB_HEARD_BY)
            d_all = DeviceArray(np.arange(n, dtype=np.int32))
            keep.append(d_all)
            ptrs = [d_all.ptr.value + 4 * PER_TICK * b for b in range(n // PER_TICK)]
            print("%d nodes: yardstick" % n, file=sys.stderr, flush=True)
            routes(prm)
            got, tot, links = yardstick(eng, n, ptrs, prm)
            assert (got["cost"] == DeviceArray.read(d_cost.ptr.value, np.uint64, n)).all()
            assert (got["parent"] == DeviceArray.read(d_par.ptr.value, np.int32, n)).all()
            out["yardstick"] = dict(timed(lambda: yardstick(eng, n, ptrs, prm), max(3, reps // 4), warm=1), batch_ticks=min(rsa.MAX_BATCH, n // PER_TICK),
                                    per_tick=PER_TICK, link_capacity_per_tick=LINK_CAP, links=links, direction="heard_by")
    finally:
        for d in keep:
            d.free()
        eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0]) if args else 10)
    out = {"unit": "us per query; kernels: summed dispatch intervals per query", "air_us_of_the_cost": 4064, "max_link_cost": 1024,
           "marginal_sensitivity_dbm": SENS_MARGINAL, "shapes": []}
    for n in (100_000, 1_000_000):
        out["shapes"].append(shape(n, reps, with_yardstick=n == 100_000))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
