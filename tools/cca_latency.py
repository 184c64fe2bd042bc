"""Latency of the carrier-sense gated tick (rm_tick_run_sources_cca*) at BASELINE configs[4]'s shape: 1 M nodes, the
SINR medium, 1000 new frames of 8128 us per 1000 us tick.  Before every measured call eight ungated ticks bring the on-air window
back to its steady size (8000 frames live when the next tick begins), so that every call of every row sees a window of the same
make-up; the measured call is the tick after them, with 1000 candidates, sampled 50 us into the tick, frames starting at 100 us.

  gated_tick          rm_tick_run_sources_cca_device, host clock around call + stream synchronise
  ungated_tick        rm_tick_run_sources_device over the same list, the yardstick
  host_sequence       what the gated tick replaces: rm_channel_energy on the list, filter on the host, upload, plain tick
  kernels_us          dispatch intervals (rm_profile_kernels) of k_cca_gate<true> and, on the same list and window (a query issued
                      right before the gated tick), of k_energy_sum<true>; k_energy_index<true> for scale

Medians of `reps` with min and max, all in one process.  Prints one JSON line.  Run on the GPU box:  python tools/cca_latency.py [reps]
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

THRESHOLD = -90.0


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def main():
    reps = max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 40)
    cfg = W.CONFIGS["c5"]
    n, t = cfg["n"], W.tx_count(cfg)
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(1 << 22)
    pool = 32
    host = [W.choose_sources(n, t, 0xC0FFEE00 + cfg["index"], k) for k in range(pool)]
    dev = [DeviceArray(h) for h in host]
    d_f, d_e, d_tmp = DeviceArray(nbytes=t), DeviceArray(nbytes=8 * t), DeviceArray(nbytes=4 * t)
    hip = C.CDLL("libamdhip64.so.7")
    tick = [0]

    def times():
        t0 = tick[0] * W.TICK_US
        tick[0] += 1
        return t0, t0 + 50, t0 + 100

    def ungated():
        k = tick[0]
        t0, _, ts = times()
        eng.tick_run_sources_device(t0, t0 + W.TICK_US, dev[k % pool].ptr.value, t, ts, W.AIR_US)

    def gated():
        k = tick[0]
        t0, tc, ts = times()
        eng.tick_run_sources_cca_device(t0, t0 + W.TICK_US, dev[k % pool].ptr.value, t, ts, W.AIR_US, tc, THRESHOLD, d_f.ptr.value, d_e.ptr.value)

    def host_sequence():
        k = tick[0]
        t0, tc, ts = times()
        _, flags = eng.channel_energy(tc, nodes=host[k % pool], cca_threshold_dbm=THRESHOLD)
        lst = np.where(flags != 0, -1, host[k % pool]).astype(np.int32)
        assert hip.hipMemcpy(d_tmp.ptr, C.c_void_p(lst.ctypes.data), C.c_size_t(lst.nbytes), 1) == 0
        eng.tick_run_sources_device(t0, t0 + W.TICK_US, d_tmp.ptr.value, t, ts, W.AIR_US)

    def refill():
        for _ in range(8):
            ungated()
        eng.sync()

    def timed(fn):
        us = []
        for rep in range(reps + 5):          # (five warm-up calls)
            refill()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            if rep >= 5:
                us.append((time.perf_counter() - t0) * 1e6)
        return stats(us)

    for _ in range(24):
        ungated()
    eng.sync()
    out = {"nodes": n, "candidates": t, "air_us": W.AIR_US, "frames_live_when_the_tick_begins": 8 * t, "threshold_dbm": THRESHOLD}
    out["gated_tick"] = timed(gated)
    out["deferred_share"] = float((DeviceArray.read(d_f.ptr.value, np.uint8, t) != 0).mean())
    out["ungated_tick"] = timed(ungated)
    out["host_sequence"] = timed(host_sequence)
    out["gated_tick_again"] = timed(gated)
    # the kernels' own dispatch intervals, call by call: the query's sum and the gate over the same list and the same window
    per = {"k_cca_gate<true>": [], "k_energy_sum<true>": [], "k_energy_index<true>": []}
    for rep in range(reps):
        refill()
        k = tick[0]
        eng.profile_enable(1)
        eng.channel_energy_device(k * W.TICK_US + 50, dev[k % pool].ptr.value, t, None, THRESHOLD, d_e.ptr.value, d_f.ptr.value)
        gated()
        eng.sync()
        for name, v in eng.profile_kernels().items():
            if name in per:
                per[name].append(v[1] * 1e3 / max(v[0], 1))
        eng.profile_enable(0)
    out["kernels_us"] = {name: stats(v) for name, v in per.items() if v}
    print(json.dumps(out))
    for d in dev + [d_f, d_e, d_tmp]:
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
