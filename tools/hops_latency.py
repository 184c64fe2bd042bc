"""Latency of the hop query (rm_hops.hip) at the bench's 100 k and 1 M node shapes (the log-distance medium with
shadowing, BASELINE configs[2]'s field), one root (node 0), every potential link, both directions.  One process.

  query               rm_hops_query_device into device buffers (hop, parent, rssi, children): host clock around the call, which
                      returns with the outputs complete
  kernels             the kernels' own dispatch intervals (rm_profile_kernels) summed per query, and their launches per query, in
                      runs of their own
  yardstick           (100 k nodes only) the one route to the levels without the query: a flood by lone ticks --
                      rm_tick_run_sources_device with level L's nodes as sources, the result copied to the host, the host keeps the
                      labels and uploads the next level.  With every radio on this is the RM_NB_HEARS tree's levels; they are
                      compared with the query's once, before anything is timed.  It gives no parents.

Medians of `reps` runs after two warm-up runs, with min and max.  Prints one JSON line.
Run on the GPU box:  python tools/hops_latency.py [reps]
"""
import ctypes as C
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
LINK_CAP = 1 << 23
CLOCK = [0]   # every lone tick takes the next tick in time


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


def flood(eng, n, d_level):
    """the levels from node 0 through lone ticks -> hop [n]"""
    label = np.full(n, -1, dtype=np.int32)
    label[0] = 0
    level, L = np.zeros(1, dtype=np.int32), 0
    while len(level):
        assert d_level._hip.hipMemcpy(d_level.ptr, C.c_void_p(level.ctypes.data), C.c_size_t(level.nbytes), 1) == 0   # H2D
        t0 = CLOCK[0]
        CLOCK[0] += TICK
        eng.tick_run_sources_device(t0, t0 + TICK, d_level.ptr.value, len(level), t0, AIR)
        res = eng.result_copy(len(level), cap=LINK_CAP)
        assert res.count < LINK_CAP
        nxt = np.unique(res.dst)
        level = nxt[label[nxt] == -1].astype(np.int32)
        label[level] = L + 1
        L += 1
    return label


def shape(n, reps, with_yardstick):
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    assert np.asarray(nodes.enabled).all()   # (the flood is the HEARS tree only with every radio on)
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(LINK_CAP)
    d_hop, d_par, d_rssi, d_chl = DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n), DeviceArray(nbytes=8 * n), DeviceArray(nbytes=4 * n)
    d_root, d_level = DeviceArray(np.zeros(1, dtype=np.int32)), DeviceArray(nbytes=4 * n)
    keep = [d_hop, d_par, d_rssi, d_chl, d_root, d_level]
    out = {"nodes": n, "roots": 1}
    try:
        def query(direction):
            return eng.hops_device(direction, d_root.ptr.value, 1, d_hop.ptr.value, d_par.ptr.value, d_rssi.ptr.value, d_chl.ptr.value)

        if with_yardstick:
            query(rsa.NB_HEARS)
            hop = DeviceArray.read(d_hop.ptr.value, np.int32, n)
            assert (flood(eng, n, d_level) == hop).all()
            out["yardstick"] = dict(timed(lambda: flood(eng, n, d_level), max(3, reps // 2), warm=1), link_capacity=LINK_CAP, direction="hears")
        for name, d in (("heard_by", rsa.NB_HEARD_BY), ("hears", rsa.NB_HEARS)):
            o = dict(query(d))
            o["query"] = timed(lambda: query(d), reps)
            per, launches = {}, {}
            for rep in range(reps):
                eng.profile_enable(1)
                query(d)
                for kname, v in eng.profile_kernels().items():
                    if kname.startswith("k_hop_") or kname.startswith("k_nb_"):
                        per.setdefault(kname, []).append(v[1] * 1e3)
                        launches[kname] = int(v[0])
                eng.profile_enable(0)
            o["kernels"] = {kname: dict(stats(v), launches=launches[kname]) for kname, v in per.items()}
            out[name] = o
    finally:
        for d in keep:
            d.free()
        eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0]) if args else 10)
    out = {"unit": "us per query; kernels: summed dispatch intervals per query", "air_us": AIR, "shapes": []}
    for n in (100_000, 1_000_000):
        out["shapes"].append(shape(n, reps, with_yardstick=n == 100_000))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
