"""Latency of the neighbour query (rm_neighbors.hip) at the bench's 100 k and 1 M node shapes (the log-distance
medium with shadowing, BASELINE configs[2]'s field), K = 8, both directions.  One process.

  all_nodes           rm_neighbors_query_device over all nodes into device buffers: host clock around the call plus a stream
                      synchronise
  k_nb_*              the kernels' own dispatch intervals (rm_profile_kernels), per query, in runs of their own
  list_1000           the same for a device list of 1000 random nodes
  yardstick           (100 k nodes only) the only route to these rows without the query: every node as a source through
                      rm_batch_run_sources_device in batches of `batch_ticks` ticks of `per_tick` sources, rm_batch_result_view,
                      rm_neighbors_from_result per slot; host clock around all of it.  It gives the HEARD_BY rows; they are compared
                      with the query's once, before anything is timed.  The medium has no SINR: the frames of a tick do not
                      change each other's heard links.

Medians of `reps` runs after two warm-up runs, with min and max.  Prints one JSON line.
Run on the GPU box:  python tools/neighbors_latency.py [reps]
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

K = 8
TICK = W.TICK_US
AIR = 640
PER_TICK, LINK_CAP = 1000, 1 << 20
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


def yardstick(eng, n, ptrs):
    """all HEARD_BY rows through the evaluating path -> peer [n][K], degree [n]"""
    peer, degree = np.empty((n, K), dtype=np.int32), np.empty(n, dtype=np.int32)
    n_ticks = n // PER_TICK
    for b0 in range(0, n_ticks, rsa.MAX_BATCH):
        nb = min(rsa.MAX_BATCH, n_ticks - b0)
        t0 = [CLOCK[0] + TICK * b for b in range(nb)]
        CLOCK[0] += TICK * nb
        eng.batch_run_sources_device(t0, [t + TICK for t in t0], ptrs[b0:b0 + nb], [PER_TICK] * nb, t0, [AIR] * nb)
        res, _ = eng.batch_result_view(nb)
        for b, r in enumerate(res):
            rows = rsa.Engine.neighbors_from_result(r, K, fields=("degree",))
            at = (b0 + b) * PER_TICK
            peer[at:at + PER_TICK], degree[at:at + PER_TICK] = rows["peer"], rows["degree"]
    return peer, degree


def shape(n, reps, with_yardstick):
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(LINK_CAP)
    d_peer, d_rssi, d_deg = DeviceArray(nbytes=4 * n * K), DeviceArray(nbytes=8 * n * K), DeviceArray(nbytes=4 * n)
    some = np.random.default_rng(16).choice(n, 1000, replace=False).astype(np.int32)
    d_some = DeviceArray(some)
    keep = [d_peer, d_rssi, d_deg, d_some]
    out = {"nodes": n, "K": K}
    try:
        def query(direction, lst=None):
            eng.neighbors_device(direction, K, d_peer.ptr.value, d_rssi.ptr.value, d_deg.ptr.value, None if lst is None else d_some.ptr.value,
                                 None if lst is None else len(some))
            eng.sync()

        query(rsa.NB_HEARD_BY)
        deg = DeviceArray.read(d_deg.ptr.value, np.int32, n)
        out["mean_degree"] = float(deg.mean())
        if with_yardstick:
            order = np.arange(n, dtype=np.int32)
            d_all = DeviceArray(order)
            keep.append(d_all)
            ptrs = [d_all.ptr.value + 4 * PER_TICK * b for b in range(n // PER_TICK)]
            peer, degree = yardstick(eng, n, ptrs)
            assert (degree == deg).all() and (peer == DeviceArray.read(d_peer.ptr.value, np.int32, n * K).reshape(n, K)).all()
            out["yardstick"] = dict(timed(lambda: yardstick(eng, n, ptrs), max(3, reps // 4), warm=1), batch_ticks=min(rsa.MAX_BATCH, n // PER_TICK),
                                    per_tick=PER_TICK, link_capacity_per_tick=LINK_CAP, links=int(deg.sum()))
        for name, d in (("heard_by", rsa.NB_HEARD_BY), ("hears", rsa.NB_HEARS)):
            o = {"all_nodes": timed(lambda: query(d), reps), "list_1000": timed(lambda: query(d, some), reps)}
            per = {}
            for rep in range(reps):
                eng.profile_enable(1)
                query(d)
                for kname, v in eng.profile_kernels().items():
                    if kname.startswith("k_nb_"):
                        per.setdefault(kname, []).append(v[1] * 1e3 / max(v[0], 1))
                eng.profile_enable(0)
            o["kernels"] = {kname: stats(v) for kname, v in per.items()}
            out[name] = o
    finally:
        for d in keep:
            d.free()
        eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0]) if args else 20)
    out = {"unit": "us per query", "air_us": AIR, "shapes": []}
    for n in (100_000, 1_000_000):
        out["shapes"].append(shape(n, reps, with_yardstick=n == 100_000))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
