"""Per-tick cost of the reception stage behind batched ticks: rm_batch_run_sources_device + rm_events_process_batch
(deliveries to the host) on the configs[2] shape (100 k nodes, 1 000 frames of 8 128 us per 1 000 us tick, shadowing),
next to the lone closed loop of tools/events_latency.py c3 (rm_tick_run_sources_device + rm_events_process) from the same
process.  Run on the GPU box:  python tools/batch_events_latency.py [batch] [batches] [lone_ticks]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import radio_sim_amd as rsa  # noqa: E402
from radio_sim_amd import workload as W  # noqa: E402
from util import DeviceArray  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 64
batches = int(sys.argv[2]) if len(sys.argv) > 2 else 8
lone_ticks = int(sys.argv[3]) if len(sys.argv) > 3 else 200
idx, n = 3, 100_000
t = n // 100
nodes = W.make_nodes(n, idx)
kind_name, kw = W.model_kwargs("logdist_shadow")
eng = rsa.Engine(0)
eng.upload_table(nodes)
eng.set_model(rsa.MODEL_LOGDIST, **kw)
eng.set_link_capacity(1 << 21)
devs = [DeviceArray(W.choose_sources(n, t, 0xC0FFEE00 + idx, k)) for k in range(32)]


def lone(k0, k1):
    got = 0
    for k in range(k0, k1):
        eng.tick_run_sources_device(k * 1000, k * 1000 + 1000, devs[k % 32].ptr.value, t, k * 1000, W.AIR_US)
        got += len(eng.events_process(k * 1000 + 1000, copy=False, runs=True)[3])
    return got


def batched(j0, j1):
    got, issue, hand = 0, 0.0, 0.0
    for j in range(j0, j1):
        starts = [(j * batch + b) * 1000 for b in range(batch)]
        ends = [s + 1000 for s in starts]
        ptrs = [devs[(j * batch + b) % 32].ptr.value for b in range(batch)]
        t0 = time.perf_counter()
        eng.batch_run_sources_device(starts, ends, ptrs, [t] * batch, starts, [W.AIR_US] * batch)
        t1 = time.perf_counter()
        views = eng.events_process_batch(ends, copy=False, runs=True)
        t2 = time.perf_counter()
        got += sum(len(v[3]) for v in views)
        issue += t1 - t0
        hand += t2 - t1
    return got, issue, hand


eng.events_enable(1 << 16, 1 << 21)
eng.set_time(0)                     # (a new Simulator starts at time 0)
batched(0, 2)                       # warm-up: the host-mapped block reaches its size
t0 = time.perf_counter()
got, issue, hand = batched(2, 2 + batches)
dt = (time.perf_counter() - t0) / (batches * batch)
eng.events_enable(1 << 16, 1 << 21)
eng.set_time(0)                     # (a new Simulator starts at time 0)
lone(0, 24)
t1 = time.perf_counter()
got_lone = lone(24, 24 + lone_ticks)
dt_lone = (time.perf_counter() - t1) / lone_ticks
print(json.dumps({"workload": "configs[2] (c3)", "batch": batch, "us_per_tick": dt * 1e6, "deliveries_per_tick": got / (batches * batch),
                  "host_batch_run_us_per_batch": issue / batches * 1e6, "host_events_process_batch_us_per_batch": hand / batches * 1e6,
                  "lone_us_per_tick": dt_lone * 1e6, "lone_deliveries_per_tick": got_lone / lone_ticks}))
eng.close()
