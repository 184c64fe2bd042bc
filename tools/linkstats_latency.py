"""Latency of the watched-link statistics' pass (rm_linkstats.hip) at the batch shape of BASELINE.json configs[2]: 100 k
nodes, log-distance with log-normal shadowing, 1000 frames per tick, 128 ticks per batch (bench.py's own batch size for that
configuration; ticks of this medium are self-contained).  K = 8, and every node watches the first eight distinct sources it hears
in the measured batch (in tick order, then link order), taken from the batch's own results.  Per BATCH:

  batch_off           rm_batch_run_sources_device with the feature off, host clock around call + stream synchronise
  batch_on            the same with rm_linkstats_enable(ctx, 8) and the rows above
  batch_on_empty      the same with K = 8 and every slot empty (the pass reads pkt, the record, dst and the peer row; no atomics)
  pass_us             dispatch interval (rm_profile_kernels) of k_linkstats_batch in batch_on, per batch
  links_per_batch, matched_per_batch     heard links of one batch, and those the pass adds to an entry (up to six atomics each)

The no-regression check of the "off" path: run this tool with --off-only and RM_LIBRARY=<the parent commit's build> in the same
session (it prints batch_off alone, twice); this change's batch_off median has to lie inside the parent's min .. max.
Medians of `reps` (20 at least) after three warm-up calls, with min and max, all series in one process.  Prints one JSON line.  Run on
the GPU box:  python tools/linkstats_latency.py [reps] [--off-only]
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

BATCH = 128
K = 8


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def first_heard_rows(n, k, src, dst):
    """per node the first k distinct sources among its heard links (src, dst in tick order, then link order): int32 [n][k]"""
    key = dst.astype(np.int64) * n + src.astype(np.int64)
    _, first = np.unique(key, return_index=True)          # the first link of every distinct (dst, src)
    order = first[np.lexsort((first, dst[first]))]        # by receiver, then by first occurrence
    d = dst[order]
    rank = np.arange(len(d)) - np.searchsorted(d, d, side="left")
    keep = rank < k
    rows = np.full((n, k), -1, dtype=np.int32)
    rows[d[keep], rank[keep]] = src[order][keep]
    return rows


def main():
    off_only = "--off-only" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if off_only:                                  # a library of before E14 has none of its entry points
        from radio_sim_amd import _lib
        for name in [k for k in _lib.SIGNATURES if k.startswith("rm_linkstats_")]:
            del _lib.SIGNATURES[name]
    reps = max(20, int(args[0]) if args else 20)
    cfg = W.CONFIGS["c3"]
    n, t = cfg["n"], W.tx_count(cfg)
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    eng.upload_table(nodes)
    eng.set_model(rsa.MODEL_LOGDIST, **kw)
    srcs = [W.choose_sources(n, t, 0xC0FFEE00 + cfg["index"], k) for k in range(BATCH)]
    dev = [DeviceArray(s) for s in srcs]
    tb = [b * W.TICK_US for b in range(BATCH)]

    def batch():
        eng.batch_run_sources_device(tb, [x + W.TICK_US for x in tb], [d.ptr.value for d in dev], [t] * BATCH, tb, [W.AIR_US] * BATCH)

    def timed():
        us = []
        for rep in range(reps + 3):          # (three warm-up calls)
            t0 = time.perf_counter()
            batch()
            eng.sync()
            if rep >= 3:
                us.append((time.perf_counter() - t0) * 1e6)
        return stats(us)

    batch()
    eng.sync()
    out = {"nodes": n, "frames_per_tick": t, "ticks_per_batch": BATCH, "K": K, "unit": "us per batch"}
    out["batch_off"] = timed()
    if off_only:
        out["batch_off_again"] = timed()
        print(json.dumps(out))
        return
    # the watch rows from the batch's own results
    s_all, d_all = [], []
    for b in range(BATCH):
        r = eng.batch_result_copy(b, t, cap=1 << 20)
        s_all.append(srcs[b][r.pkt])
        d_all.append(r.dst.copy())
    src, dst = np.concatenate(s_all), np.concatenate(d_all)
    rows = first_heard_rows(n, K, src, dst)
    out["links_per_batch"] = int(len(dst))
    eng.linkstats_enable(K)
    out["batch_on_empty"] = timed()
    eng.linkstats_watch(rows)
    out["batch_on"] = timed()
    # what one batch adds: cleared entries, one batch, read back
    eng.linkstats_reset()
    batch()
    tbl, tot = eng.linkstats_read()
    out["matched_per_batch"] = int(tbl["heard"].sum())
    out["entries_hit"] = int((tbl["heard"] > 0).sum())
    out["ticks_counted"], out["ticks_skipped"] = tot["ticks_counted"], tot["ticks_skipped"]
    per = []
    for rep in range(reps):
        eng.profile_enable(1)
        batch()
        eng.sync()
        v = eng.profile_kernels().get("k_linkstats_batch")
        if v:
            per.append(v[1] * 1e3 / max(v[0], 1))
        eng.profile_enable(0)
    out["pass_us"] = stats(per) if per else None
    eng.linkstats_enable(0)
    out["batch_off_again"] = timed()
    print(json.dumps(out))
    for d in dev:
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
