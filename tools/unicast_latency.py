"""Latency of the unicast outcome query (rm_unicast.hip) at the size of BASELINE configs[2]: 100 k nodes, the shadowed
log-distance medium, 1000 frames per tick, 64 ticks per batch, one wanted node per packet (a receiver that heard the frame for three
packets in four, another node for the fourth).  After ONE batch, alternating in one process, per repeat:

  query_device        rm_unicast_query_device over the 64 slots (64 000 entries), host clock around the call and a stream synchronise
  query_device_x16    sixteen such calls back to back, then one synchronise, per call (what a caller pays that does not wait)
  view                what the parent commit offers for the same answer, first half: rm_batch_result_view of the 64 slots
  view_and_search     ... and the second half: per packet a binary search of its segment of dst on the host (numpy, one searchsorted
                      per slot over keys packet * n_nodes + dst) for status, rssi and the reply list
  from_result         the library's own host function over the same views (rm_unicast_from_result), for comparison

Medians of `reps` (20 at least) after three warm-up rounds, with min and max.  The answers of the three ways are compared once.
Prints one JSON line; --write also writes it to profiles/unicast_latency.json, --write=PATH to PATH.  Run on the GPU box:
  python tools/unicast_latency.py [reps] [--write[=PATH]]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import radio_sim_amd as rsa  # noqa: E402
from radio_sim_amd import workload as W  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import DeviceArray  # noqa: E402

BATCH = 64
TYPES = {"status": np.uint8, "link": np.int32, "rssi": np.float64, "sinr": np.float64, "reply_src": np.int32}


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def search(views, want, n_nodes):
    """the numpy lookup over the views of rm_batch_result_view: per slot one searchsorted -> status, rssi, reply_src (flat)"""
    status, rssi, reply = [], [], []
    for r, w in zip(views, want):
        off = r.pkt_offset.astype(np.int64)
        n_pkt = len(off) - 1
        pkt = np.repeat(np.arange(n_pkt, dtype=np.int64), np.diff(off))
        key = pkt * n_nodes + r.dst
        ask = np.arange(n_pkt, dtype=np.int64) * n_nodes + w
        i = np.minimum(np.searchsorted(key, ask), max(len(key) - 1, 0))
        hit = (key[i] == ask) if len(key) else np.zeros(n_pkt, dtype=bool)
        ok = hit & (r.verdict[i] == rsa.DELIVERED)
        status.append(np.where(hit, np.where(ok, rsa.UC_DELIVERED, rsa.UC_INTERFERED), rsa.UC_UNHEARD).astype(np.uint8))
        rssi.append(np.where(hit, r.rssi[i], np.nan))
        reply.append(np.where(ok, w, -1).astype(np.int32))
    return np.concatenate(status), np.concatenate(rssi), np.concatenate(reply)


def main():
    out_path = None
    for a in sys.argv[1:]:
        if a == "--write":
            out_path = os.path.join(ROOT, "profiles", "unicast_latency.json")
        elif a.startswith("--write="):
            out_path = a.split("=", 1)[1]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(20, int(args[0]) if args else 20)
    cfg = W.CONFIGS["c3"]
    n, t = cfg["n"], W.tx_count(cfg)
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    eng.set_link_capacity(1 << 22)
    src = [W.choose_sources(n, t, 0xC0FFEE00 + cfg["index"], k) for k in range(BATCH)]
    dev = [DeviceArray(s) for s in src]
    tb = [b * W.TICK_US for b in range(BATCH)]
    eng.batch_run_sources_device(tb, [x + W.TICK_US for x in tb], [d.ptr.value for d in dev], [t] * BATCH, tb, [W.AIR_US] * BATCH)
    eng.sync()
    # the wanted nodes, from the batch's own results: a receiver that heard the frame (three in four), else another node
    rng = np.random.default_rng(12)
    want, links = [], 0
    for b in range(BATCH):
        r = eng.batch_result_copy(b, t, cap=1 << 22)
        links += r.count
        off = r.pkt_offset.astype(np.int64)
        w = rng.integers(0, n, t).astype(np.int32)
        seg = np.diff(off)
        pick = (np.arange(t) % 4 != 3) & (seg > 0)
        w[pick] = r.dst[(off[:-1] + rng.integers(0, 1 << 30, t) % np.maximum(seg, 1))[pick]]
        want.append(w)
    flat = np.concatenate(want)
    total = len(flat)
    d_want = DeviceArray(flat)
    d_out = {f: DeviceArray(np.zeros(total, dtype=dt)) for f, dt in TYPES.items()}
    ptrs = {f: d.ptr.value for f, d in d_out.items()}
    n_pkt = [t] * BATCH

    def query(k=1):
        t0 = time.perf_counter()
        for _ in range(k):
            eng.unicast_query_device(n_pkt, d_want.ptr.value, ptrs)
        eng.sync()
        return (time.perf_counter() - t0) * 1e6 / k

    def view(lookup):
        t0 = time.perf_counter()
        views, _ = eng.batch_result_view(BATCH)
        t1 = time.perf_counter()
        if lookup == "numpy":
            ans = search(views, want, n)
        else:
            ans = [rsa.Engine.unicast_from_result(r, None, n, w, fields=("status", "rssi", "reply_src")) for r, w in zip(views, want)]
        t2 = time.perf_counter()
        return (t1 - t0) * 1e6, (t2 - t0) * 1e6, ans

    series = {k: [] for k in ("query_device", "query_device_x16", "view", "view_and_search", "view_and_from_result")}
    for rep in range(reps + 3):          # (three warm-up rounds; the ways alternate inside a round)
        a = query()
        b = query(16)
        v, vs, _ = view("numpy")
        _, vf, _ = view("lib")
        if rep >= 3:
            for k, x in zip(series, (a, b, v, vs, vf)):
                series[k].append(x)
    # the three ways give one answer
    query()
    got = {f: DeviceArray.read(d_out[f].ptr.value, TYPES[f], total) for f in ("status", "rssi", "reply_src")}
    _, _, (s_np, r_np, p_np) = view("numpy")
    _, _, lib = view("lib")
    same = (np.array_equal(got["status"], s_np) and np.array_equal(got["reply_src"], p_np) and
            np.array_equal(got["rssi"].view(np.uint64)[s_np >= rsa.UC_INTERFERED], r_np.view(np.uint64)[s_np >= rsa.UC_INTERFERED]) and
            np.array_equal(got["status"], np.concatenate([x["status"] for x in lib])) and
            np.array_equal(got["reply_src"], np.concatenate([x["reply_src"] for x in lib])))
    out = {"nodes": n, "frames_per_tick": t, "ticks_per_batch": BATCH, "entries": total, "links_per_batch": int(links),
           "links_per_tick": links / BATCH, "delivered_entries": int((got["status"] == rsa.UC_DELIVERED).sum()),
           "unheard_entries": int((got["status"] == rsa.UC_UNHEARD).sum()), "answers_agree": bool(same), "unit": "us per call (64 ticks)"}
    out.update({k: stats(v) for k, v in series.items()})
    line = json.dumps(out)
    print(line)
    if out_path:
        open(out_path, "w").write(line + "\n")
    for d in dev + [d_want] + list(d_out.values()):
        d.free()
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
