"""Latency of the listening schedules' pass (rm_listen.hip) at the shape of tools/errmodel_latency.py and
tools/stats_latency.py: 1 M nodes, the SINR medium, 1000 frames per tick, frames of 8128 us over ticks of 1000 us, 64 ticks per batch.
Before every measured call eight ticks bring the on-air window back to the same steady state (8000 frames live when the next tick
begins).  Per TICK (the call's time over 64):

  batch_off           rm_batch_run_sources_device with schedules off, host clock around call + stream synchronise
  batch_zero          the same after rm_listen_set with every period 0: every delivered link leaves the pass after one load
  batch_duty          the same with a realistic schedule: every node period 125 000 us, 1 % on, random phases -- every delivered link
                      reaches the 64-bit remainder
  pass_zero_us, pass_duty_us     dispatch interval (rm_profile_kernels) of k_listen_batch in those two, per batch of 64 ticks
  links_per_batch, remainder_share, missed_per_batch     of one batch under the realistic schedule: heard links, the share of them
                      that reaches the remainder (RM_DELIVERED before the pass, at a receiver with a period), links the pass flipped

The no-regression check of the "off" path: run this tool with --off-only and RM_LIBRARY=<the parent commit's build> in the same
session (it prints batch_off alone, twice); this change's batch_off median has to lie inside the parent's min .. max.
Medians of `reps` (20 at least) after three warm-up calls, with min and max, all series in one process.  Prints one JSON line.  Run on
the GPU box:  python tools/listen_latency.py [reps] [--off-only]
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

BATCH = 64
PERIOD_US, ON_US = 125000, 1250


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def main():
    off_only = "--off-only" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if off_only:                                  # a library of before E13 has none of its entry points
        from radio_sim_amd import _lib
        for name in [k for k in _lib.SIGNATURES if k.startswith("rm_listen_")]:
            del _lib.SIGNATURES[name]
    reps = max(20, int(args[0]) if args else 20)
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
    tick = [0]

    def batch(k=BATCH):
        first = tick[0]
        tick[0] += k
        tb = [(first + b) * W.TICK_US for b in range(k)]
        eng.batch_run_sources_device(tb, [x + W.TICK_US for x in tb], [dev[(first + b) % pool].ptr.value for b in range(k)], [t] * k,
                                     [x + 100 for x in tb], [W.AIR_US] * k)

    def refill():
        batch(8)
        eng.sync()

    def timed():
        us = []
        for rep in range(reps + 3):          # (three warm-up calls)
            refill()
            t0 = time.perf_counter()
            batch()
            eng.sync()
            if rep >= 3:
                us.append((time.perf_counter() - t0) * 1e6 / BATCH)
        return stats(us)

    def pass_interval():
        per = []
        for rep in range(reps):
            refill()
            eng.profile_enable(1)
            batch()
            eng.sync()
            v = eng.profile_kernels().get("k_listen_batch")
            if v:
                per.append(v[1] * 1e3 / max(v[0], 1))
            eng.profile_enable(0)
        return stats(per) if per else None

    batch(24)
    eng.sync()
    out = {"nodes": n, "frames_per_tick": t, "ticks_per_batch": BATCH, "air_us": W.AIR_US, "frames_live_when_the_batch_begins": 8 * t,
           "unit": "us per tick", "period_us": PERIOD_US, "on_us": ON_US}
    out["batch_off"] = timed()
    if off_only:
        out["batch_off_again"] = timed()
        print(json.dumps(out))
        for d in dev:
            d.free()
        eng.close()
        return
    eng.listen_set(np.zeros((n, 3), dtype=np.int64))
    out["batch_zero"] = timed()
    out["pass_zero_us"] = pass_interval()
    duty = np.zeros((n, 3), dtype=np.int64)
    duty[:, 0], duty[:, 1] = PERIOD_US, ON_US
    duty[:, 2] = np.random.default_rng(13).integers(0, PERIOD_US, n)
    eng.listen_set(duty)
    out["batch_duty"] = timed()
    out["pass_duty_us"] = pass_interval()
    # what one batch under the realistic schedule looks like: heard links, delivered ones after the pass, links the pass flipped
    refill()
    eng.listen_missed_reset()
    eng.stats_enable()
    eng.stats_reset()
    batch()
    tbl, _ = eng.stats_read()
    missed = int(eng.listen_missed().sum())
    eng.stats_enable(False)
    out["links_per_batch"] = int(tbl["rx_heard"].sum())
    out["missed_per_batch"] = missed
    out["remainder_share"] = (float(tbl["rx_delivered"].sum()) + missed) / max(out["links_per_batch"], 1)
    eng.listen_clear()
    out["batch_off_again"] = timed()
    print(json.dumps(out))
    for d in dev:
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
