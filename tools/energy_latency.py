"""Latency of the channel energy query (rm_channel_energy*) at BASELINE configs[4]'s shape: 1 M nodes, the SINR
medium, 1000 new frames of 8128 us per 1000 us tick.  Ticks run until the on-air window is at its steady size, then

  all nodes, device form   rm_channel_energy_device over every node, stream-synchronised: median / min / max
  1000-node list           rm_channel_energy (host arrays in and out), what a lock-stepped host calls per tick
  yardsticks               one lone SINR tick by scan over the same window (k_tick_frames + k_sinr_scan, 1000 new frames);
                           rm_node_info for the same 1000 nodes (events on)

Prints one JSON line.  Run on the GPU box:  python tools/energy_latency.py [reps]
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


def stats(us):
    us = np.sort(np.asarray(us))
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
    dev = [DeviceArray(W.choose_sources(n, t, 0xC0FFEE00 + cfg["index"], k)) for k in range(pool)]
    tick = [0]

    def one_tick():
        k = tick[0]
        eng.tick_run_sources_device(k * W.TICK_US, (k + 1) * W.TICK_US, dev[k % pool].ptr.value, t, k * W.TICK_US, W.AIR_US)
        tick[0] += 1

    for _ in range(24):                      # 9 ticks of frames on the air from the ninth tick on
        one_tick()
    eng.sync()
    now = (tick[0] - 1) * W.TICK_US + 100
    d_e = DeviceArray(nbytes=8 * n)
    d_f = DeviceArray(nbytes=n)
    out = {"nodes": n, "frames_per_tick": t, "air_us": W.AIR_US, "frames_live": 9 * t}

    def timed(fn, warm=5):
        for _ in range(warm):
            fn()
        eng.sync()
        us = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            eng.sync()
            us.append((time.perf_counter() - t0) * 1e6)
        return stats(us)

    out["all_nodes_device"] = timed(lambda: eng.channel_energy_device(now, None, n, None, -90.0, d_e.ptr.value, d_f.ptr.value))
    e = DeviceArray.read(d_e.ptr.value, np.float64, n)
    out["share_above_noise"] = float((e > -100.0).mean())
    lst = np.sort(np.random.default_rng(1).choice(n, 1000, replace=False)).astype(np.int32)
    out["list_1000_host"] = timed(lambda: eng.channel_energy(now, nodes=lst, cca_threshold_dbm=-90.0))
    # yardstick: lone SINR ticks by scan over the same window, one at a time
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        one_tick()
        eng.sync()
        us.append((time.perf_counter() - t0) * 1e6)
    out["lone_sinr_tick_by_scan"] = stats(us)
    out["scan_ticks"] = int(eng.air_scan_ticks())
    now = (tick[0] - 1) * W.TICK_US + 100
    out["all_nodes_device_after"] = timed(lambda: eng.channel_energy_device(now, None, n, None, -90.0, d_e.ptr.value, d_f.ptr.value))
    # per-kernel times of a few profiled queries (the kernels' own dispatch intervals)
    eng.profile_enable(1)
    for _ in range(10):
        eng.channel_energy_device(now, None, n, None, -90.0, d_e.ptr.value, d_f.ptr.value)
    eng.sync()
    out["kernels_us"] = {k: v[1] * 1e3 / max(v[0], 1) for k, v in eng.profile_kernels().items() if k.startswith("k_energy")}
    eng.profile_enable(0)
    # yardstick: rm_node_info for the same 1000 nodes
    eng.events_enable()
    out["node_info_1000"] = timed(lambda: eng.node_info(lst))
    out["list_over_node_info"] = out["list_1000_host"]["median_us"] / out["node_info_1000"]["median_us"]
    print(json.dumps(out))
    for d in dev + [d_e, d_f]:
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
