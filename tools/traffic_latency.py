"""Latency of the traffic generator (rm_traffic.hip) against what a caller does without it, at 100 k and at 1 M
nodes, 64 and 512 windows of 1000 us per batch.  Every node has period = 100 windows, jitter = period and a random phase: 1 % of the
nodes per window, the shape of bench.py's "1 % of the nodes per tick".  One process; every batch takes the next windows in time.

  host_lists          (a) what a caller does today: the same lists built on the host with numpy from the same rule (hash, high half
                      of the product, a stable sort by window), one copy to the device, the pointer table; host clock around it
  generate            (b) rm_traffic_generate_device, a stream synchronise and one copy of count to the host
  k_traffic_*         the three kernels' own dispatch intervals (rm_profile_kernels), per batch, in runs of their own
  batch / share       (c) at 64 windows: rm_batch_run_sources_device over the generated rows (n_src = count, frames of 640 us, the
                      log-distance medium with shadowing) with a stream synchronise, and (b)'s median as a share of (b) + batch.
                      Not measured at 512 windows.

The two forms' lists are compared once per shape before anything is timed.  Medians of `reps` batches after three warm-up batches,
with min and max.  Prints one JSON line.  Run on the GPU box:  python tools/traffic_latency.py [reps]
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
PERIOD = 100 * TICK
AIR = 640
SEED = 0x7AFF1C
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def umulhi(a, b):
    """the high half of the 128-bit product of two uint64 arrays"""
    a0, a1, b0, b1 = a & M32, a >> S32, b & M32, b >> S32
    cross = ((a0 * b0) >> S32) + ((a1 * b0) & M32) + a0 * b1
    return a1 * b1 + ((a1 * b0) >> S32) + (cross >> S32)


def host_lists(period, phase, jitter, seed, first, n_ticks):
    """E15's rule with numpy for windows [first + b TICK, first + (b + 1) TICK): -> the lists end to end, count per window"""
    with np.errstate(over="ignore"):
        a, b = first, first + n_ticks * TICK
        node = np.arange(len(period), dtype=np.uint64)
        hn = W._mix(W._mix(np.uint64(seed) + W.GOLDEN) ^ node)
        k_first = np.maximum((a - phase - jitter) // period, 0)
        k_last = (b - 1 - phase) // period
        wins, nodes = [], []
        for d in range(int((k_last - k_first).max()) + 1):
            k = k_first + d
            due = phase + k * period + umulhi(W._mix(hn ^ k.astype(np.uint64)), jitter.astype(np.uint64)).astype(np.int64)
            idx = np.flatnonzero((k <= k_last) & (due >= a) & (due < b))
            wins.append((due[idx] - a) // TICK)
            nodes.append(idx)
        w, nd = np.concatenate(wins), np.concatenate(nodes)
        order = np.lexsort((nd, w))
        w, nd = w[order], nd[order]
        keep = np.ones(len(w), dtype=bool)
        keep[1:] = (w[1:] != w[:-1]) | (nd[1:] != nd[:-1])
        return nd[keep].astype(np.int32), np.bincount(w[keep], minlength=n_ticks).astype(np.int32)


def shape(hip, n, n_ticks, reps, with_batch):
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    rng = np.random.default_rng(15)
    period = np.full(n, PERIOD, dtype=np.int64)
    phase = rng.integers(0, PERIOD, n).astype(np.int64)
    jitter = period.copy()
    eng.traffic_set(np.stack([period, phase, jitter, np.zeros(n, dtype=np.int64)], axis=1))
    cap = int(n // 100 * 1.5) + 64
    d_src, d_cnt, d_host = DeviceArray(nbytes=4 * n_ticks * cap), DeviceArray(nbytes=4 * n_ticks), DeviceArray(nbytes=4 * n_ticks * cap)
    count = np.zeros(n_ticks, dtype=np.int32)
    clock = [10 * PERIOD]

    def windows():
        first = clock[0]
        clock[0] += n_ticks * TICK
        lo = first + TICK * np.arange(n_ticks, dtype=np.int64)
        return first, lo, lo + TICK

    def generate(lo, hi):
        eng.traffic_generate_device(SEED, lo, hi, cap, d_src.ptr.value, d_cnt.ptr.value)
        eng.sync()                           # (the context's stream does not synchronise with the copy's)
        assert hip.hipMemcpy(C.c_void_p(count.ctypes.data), d_cnt.ptr, C.c_size_t(count.nbytes), 2) == 0   # D2H

    def host(first):
        flat, cnt = host_lists(period, phase, jitter, SEED, first, n_ticks)
        assert hip.hipMemcpy(d_host.ptr, C.c_void_p(flat.ctypes.data), C.c_size_t(flat.nbytes), 1) == 0      # H2D
        off = np.concatenate([[0], np.cumsum(cnt[:-1])])
        return flat, cnt, [d_host.ptr.value + 4 * int(o) for o in off]

    out = {"nodes": n, "windows": n_ticks, "cap": cap}
    try:
        # the two forms give the same lists
        first, lo, hi = windows()
        flat, cnt, _ = host(first)
        generate(lo, hi)
        assert (cnt == count).all() and count.max() <= cap
        rows = DeviceArray.read(d_src.ptr.value, np.int32, n_ticks * cap).reshape(n_ticks, cap)
        assert (np.concatenate([rows[b, :count[b]] for b in range(n_ticks)]) == flat).all()
        out["sources_per_batch"] = int(count.sum())
        a_us, b_us = [], []
        for rep in range(reps + 3):          # (three warm-up batches; the two forms alternate)
            first, lo, hi = windows()
            t0 = time.perf_counter()
            host(first)
            t1 = time.perf_counter()
            generate(lo, hi)
            t2 = time.perf_counter()
            if rep >= 3:
                a_us.append((t1 - t0) * 1e6)
                b_us.append((t2 - t1) * 1e6)
        out["host_lists"], out["generate"] = stats(a_us), stats(b_us)
        per = {}
        for rep in range(reps):
            first, lo, hi = windows()
            eng.profile_enable(1)
            generate(lo, hi)
            for name, v in eng.profile_kernels().items():
                if name.startswith("k_traffic"):
                    per.setdefault(name, []).append(v[1] * 1e3 / max(v[0], 1))
            eng.profile_enable(0)
        out["kernels"] = {name: stats(v) for name, v in per.items()}
        if with_batch:
            eng.set_link_capacity(1 << 20)
            c_us = []
            for rep in range(reps + 3):
                first, lo, hi = windows()
                generate(lo, hi)
                ptrs = [d_src.ptr.value + 4 * b * cap for b in range(n_ticks)]
                t0 = time.perf_counter()
                eng.batch_run_sources_device(lo, hi, ptrs, count.tolist(), lo, [AIR] * n_ticks)
                eng.sync()
                if rep >= 3:
                    c_us.append((time.perf_counter() - t0) * 1e6)
            out["batch"] = stats(c_us)
            out["generate_share_of_generate_plus_batch"] = out["generate"]["median_us"] / (out["generate"]["median_us"] + out["batch"]["median_us"])
            out["links_last_batch"] = int(sum(eng.batch_result_count(b)[0] for b in range(n_ticks)))
    finally:
        for d in (d_src, d_cnt, d_host):
            d.free()
        eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(10, int(args[0]) if args else 20)
    hip = C.CDLL("libamdhip64.so.7")
    out = {"unit": "us per batch", "period_us": PERIOD, "jitter_us": PERIOD, "window_us": TICK, "air_us": AIR, "shapes": []}
    for n in (100_000, 1_000_000):
        for n_ticks in (64, 512):
            out["shapes"].append(shape(hip, n, n_ticks, reps, with_batch=n_ticks == 64))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
