"""Latency of the carrier-sense gated batch (rm_batch_run_sources_cca_device) at BASELINE configs[4]'s shape: 1 M nodes,
the SINR medium, 1000 candidates per tick, frames of 8128 us over ticks of 1000 us, 64 ticks per batch, threshold -90 dBm, sampled 50 us
into each tick, frames starting at 100 us.  Before every measured call eight ungated ticks bring the on-air window back to the same
steady state (8000 frames live when the next tick begins).  Per TICK (the call's time over 64):

  gated_batch         (a) rm_batch_run_sources_cca_device, host clock around call + stream synchronise
  gated_lone_ticks    (b) the same 64 ticks as rm_tick_run_sources_cca_device calls back to back, one synchronise at the end: the yardstick
  ungated_batch       (c) rm_batch_run_sources_device over the same lists; (a) - (c) is the price of gating in a batch
  kernels_us          dispatch intervals (rm_profile_kernels) of the gate's kernels, per batch of 64 ticks
  deferred_share      candidates of the gated batch that deferred

Medians of `reps` with min and max, all series in one process.  Prints one JSON line.  Run on the GPU box:
python tools/cca_batch_latency.py [reps]
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

THRESHOLD = -90.0
BATCH = 64


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def main():
    reps = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20)
    cfg = W.CONFIGS["c5"]
    n, t = cfg["n"], W.tx_count(cfg)
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(1 << 22)
    pool = 96
    dev = [DeviceArray(W.choose_sources(n, t, 0xC0FFEE00 + cfg["index"], k)) for k in range(pool)]
    d_f, d_e = DeviceArray(nbytes=BATCH * t), DeviceArray(nbytes=8 * BATCH * t)
    tick = [0]

    def span(k):
        first = tick[0]
        tick[0] += k
        tb = [(first + b) * W.TICK_US for b in range(k)]
        return first, tb, [x + W.TICK_US for x in tb], [x + 50 for x in tb], [x + 100 for x in tb]

    def ungated_batch(k=BATCH):
        first, tb, te, _, ts = span(k)
        eng.batch_run_sources_device(tb, te, [dev[(first + b) % pool].ptr.value for b in range(k)], [t] * k, ts, [W.AIR_US] * k)

    def gated_batch():
        first, tb, te, tc, ts = span(BATCH)
        eng.batch_run_sources_cca_device(tb, te, [dev[(first + b) % pool].ptr.value for b in range(BATCH)], [t] * BATCH, ts, [W.AIR_US] * BATCH, tc,
                                         THRESHOLD, d_f.ptr.value, d_e.ptr.value)

    def gated_lone_ticks():
        first, tb, te, tc, ts = span(BATCH)
        for b in range(BATCH):
            eng.tick_run_sources_cca_device(tb[b], te[b], dev[(first + b) % pool].ptr.value, t, ts[b], W.AIR_US, tc[b], THRESHOLD, d_f.ptr.value + b * t,
                                            d_e.ptr.value + 8 * b * t)

    def refill():
        ungated_batch(8)
        eng.sync()

    def timed(fn):
        us = []
        for rep in range(reps + 3):          # (three warm-up calls)
            refill()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            if rep >= 3:
                us.append((time.perf_counter() - t0) * 1e6 / BATCH)
        return stats(us)

    ungated_batch(24)
    eng.sync()
    out = {"nodes": n, "candidates_per_tick": t, "ticks_per_batch": BATCH, "air_us": W.AIR_US, "frames_live_when_the_batch_begins": 8 * t,
           "threshold_dbm": THRESHOLD, "unit": "us per tick"}
    out["gated_batch"] = timed(gated_batch)
    flags = DeviceArray.read(d_f.ptr.value, np.uint8, BATCH * t)
    out["deferred_share"] = float((flags != 0).mean())
    out["gated_lone_ticks"] = timed(gated_lone_ticks)
    out["deferred_share_lone_ticks"] = float((DeviceArray.read(d_f.ptr.value, np.uint8, BATCH * t) != 0).mean())
    out["ungated_batch"] = timed(ungated_batch)
    out["gated_batch_again"] = timed(gated_batch)
    per = {}
    for rep in range(reps):
        refill()
        eng.profile_enable(1)
        gated_batch()
        eng.sync()
        for name, v in eng.profile_kernels().items():
            if name.startswith("k_ccab"):
                per.setdefault(name, []).append(v[1] * 1e3 / max(v[0], 1))
        eng.profile_enable(0)
    out["kernels_us"] = {name: stats(v) for name, v in per.items()}
    out["kernels_us_sum_of_medians"] = float(sum(s["median_us"] for s in out["kernels_us"].values()))
    print(json.dumps(out))
    for d in dev + [d_f, d_e]:
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
