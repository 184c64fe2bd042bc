"""Latency of the CSMA-CA gated batch (rm_batch_run_sources_csma_device) at the shape of tools/cca_batch_latency.py: 1 M nodes,
the SINR medium, 1000 candidates per tick, frames of 8128 us over ticks of 1000 us, 64 ticks per batch, threshold -90 dBm, sampled 50 us
into each tick, frames starting at 100 us; CSMA parameters 4, 1, 3.  Before every measured call eight ungated ticks bring the on-air
window back to the same steady state (8000 frames live when the next tick begins).  Per TICK (the call's time over 64):

  csma_batch          (a) rm_batch_run_sources_csma_device, host clock around call + stream synchronise
  host_loop           (b) what a caller does without it, the yardstick: the same 64 ticks as rm_tick_run_sources_cca host-form calls; between
                      the calls the host reads the flags, applies the backoff schedule (vectorised) and builds the next tick's list (own
                      entries, then the retries; a node's second slot of a tick is left out: the lone gate takes distinct nodes)
  gated_batch         (c) rm_batch_run_sources_cca_device over the original lists; (a) - (c) is the price of the retries
  kernels_us          dispatch intervals (rm_profile_kernels) of the gate's kernels in (a), per batch of 64 ticks
  expanded_slots, deferred_share   of the CSMA batch: slots of all expanded lists; made attempts that deferred
  carry_n0            (d) rm_batch_run_sources_csma_carry_device with an empty carry list: the no-regression check against
                      (a) of the parent commit's library, measured in the same session by running this tool with --e8-only and
                      RM_LIBRARY=<the parent's build>, which prints series (a) alone
  carry_2x32_collect  (e) the same 64 ticks as two carry batches of 32, each followed by rm_csma_carry_collect_device, the second fed
                      the first one's carry-out; carried_into_second_half: its length
  collect_kernels_us  dispatch intervals of k_csma_collect<false>, k_csma_collect_scan, k_csma_collect<true> in (e), per collect

Medians of `reps` with min and max, all series in one process.  Prints one JSON line.  Run on the GPU box:
python tools/csma_batch_latency.py [reps]
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
MAX_BACKOFFS, MIN_BE, MAX_BE, SEED = 4, 1, 3, 7


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def main():
    e8_only = "--e8-only" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if e8_only:                                  # a library of before E9 has none of its entry points
        from radio_sim_amd import _lib
        for name in [k for k in _lib.SIGNATURES if "carry" in k]:
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
    host = [W.choose_sources(n, t, 0xC0FFEE00 + cfg["index"], k) for k in range(pool)]
    dev = [DeviceArray(s) for s in host]
    d_f, d_e = DeviceArray(nbytes=BATCH * t), DeviceArray(nbytes=8 * BATCH * t)
    d_st, d_at = DeviceArray(nbytes=BATCH * t), DeviceArray(nbytes=BATCH * t)
    params = eng.csma_params(MAX_BACKOFFS, MIN_BE, MAX_BE, SEED)
    seed_mixed = mix64(np.array([SEED], dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))[0]
    tick = [0]
    np.seterr(over="ignore")

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

    last = {}

    def csma_batch():
        first, tb, te, tc, ts = span(BATCH)
        last["n_exp"] = eng.batch_run_sources_csma_device(tb, te, [dev[(first + b) % pool].ptr.value for b in range(BATCH)], [t] * BATCH, ts,
                                                          [W.AIR_US] * BATCH, tc, THRESHOLD, params,
                                                          {"status": d_st.ptr.value, "attempts": d_at.ptr.value, "flags": d_f.ptr.value})

    d_tk = DeviceArray(nbytes=4 * BATCH * t)
    d_cst, d_cat, d_ctk = DeviceArray(nbytes=BATCH * t), DeviceArray(nbytes=BATCH * t), DeviceArray(nbytes=4 * BATCH * t)

    def carry_n0():
        first, tb, te, tc, ts = span(BATCH)
        eng.batch_run_sources_csma_carry_device(tb, te, [dev[(first + b) % pool].ptr.value for b in range(BATCH)], [t] * BATCH, ts,
                                                [W.AIR_US] * BATCH, tc, THRESHOLD, params, None,
                                                {"status": d_st.ptr.value, "attempts": d_at.ptr.value, "flags": d_f.ptr.value}, None)

    def carry_halves():
        first, tb, te, tc, ts = span(BATCH)
        own = {"status": d_st.ptr.value, "attempts": d_at.ptr.value, "tick": d_tk.ptr.value}
        car = {"status": d_cst.ptr.value, "attempts": d_cat.ptr.value, "tick": d_ctk.ptr.value}
        carry, h = None, BATCH // 2
        for lo in (0, h):
            ptrs = [dev[(first + b) % pool].ptr.value for b in range(lo, lo + h)]
            eng.batch_run_sources_csma_carry_device(tb[lo:lo + h], te[lo:lo + h], ptrs, [t] * h, ts[lo:lo + h], [W.AIR_US] * h, tc[lo:lo + h],
                                                    THRESHOLD, params, carry, own, car)
            carry = eng.csma_carry_collect_device(ptrs, [t] * h, tc[lo:lo + h], carry, own, car)
            if lo == 0:
                last["carried"] = len(carry)

    def host_loop():
        first, tb, te, tc, ts = span(BATCH)
        retries = [[] for _ in range(BATCH)]          # per tick: (nodes, h1 of the origin tick, origin slot, attempt) arrays
        for b in range(BATCH):
            own = host[(first + b) % pool]
            h1_own = mix64(np.full(1, seed_mixed, dtype=np.uint64) ^ np.array([tc[b]], dtype=np.int64).view(np.uint64))[0]
            parts = [(own, np.full(len(own), h1_own, dtype=np.uint64), np.arange(len(own), dtype=np.uint64), np.zeros(len(own), dtype=np.int64))] + retries[b]
            src = np.concatenate([p[0] for p in parts])
            h1 = np.concatenate([p[1] for p in parts])
            k = np.concatenate([p[2] for p in parts])
            a = np.concatenate([p[3] for p in parts])
            _, first_at = np.unique(src, return_index=True)
            dup = np.ones(len(src), dtype=bool)
            dup[first_at] = False
            flags, _ = eng.tick_run_sources_cca(tb[b], te[b], np.where(dup, -1, src).astype(np.int32), ts[b], W.AIR_US, tc[b], THRESHOLD)
            again = ((flags != 0) | dup) & (a < MAX_BACKOFFS)
            if again.any():
                be = np.minimum(MIN_BE + a[again], MAX_BE).astype(np.uint64)
                h2 = mix64(h1[again] ^ ((k[again] << np.uint64(8)) | a[again].astype(np.uint64)))
                nxt = b + 1 + np.where(be == 0, 0, h2 >> (np.uint64(64) - np.maximum(be, np.uint64(1)))).astype(np.int64)
                for T in np.unique(nxt[nxt < BATCH]):
                    m = nxt == T
                    retries[int(T)].append((src[again][m], h1[again][m], k[again][m], a[again][m] + 1))

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
           "threshold_dbm": THRESHOLD, "csma": [MAX_BACKOFFS, MIN_BE, MAX_BE, SEED], "unit": "us per tick"}
    out["csma_batch"] = timed(csma_batch)
    if e8_only:
        out["csma_batch_again"] = timed(csma_batch)
        print(json.dumps(out))
        return
    status = DeviceArray.read(d_st.ptr.value, np.uint8, BATCH * t)
    attempts = DeviceArray.read(d_at.ptr.value, np.uint8, BATCH * t).astype(np.int64)
    out["expanded_slots"] = int(np.sum(last["n_exp"]))
    out["status_counts_none_sent_failed_pending"] = np.bincount(status, minlength=4).tolist()
    out["deferred_share"] = float((attempts.sum() - (status == 1).sum()) / max(attempts.sum(), 1))
    out["host_loop"] = timed(host_loop)
    out["gated_batch"] = timed(gated_batch)
    out["csma_batch_again"] = timed(csma_batch)
    out["carry_n0"] = timed(carry_n0)
    out["carry_2x32_collect"] = timed(carry_halves)
    out["carried_into_second_half"] = last["carried"]
    col = {}
    for rep in range(reps):
        refill()
        eng.profile_enable(1)
        carry_halves()
        eng.sync()
        for name, v in eng.profile_kernels().items():
            if name.startswith("k_csma_collect"):
                col.setdefault(name, []).append(v[1] * 1e3 / max(v[0], 1))
        eng.profile_enable(0)
    out["collect_kernels_us"] = {name: stats(v) for name, v in col.items()}
    per = {}
    for rep in range(reps):
        refill()
        eng.profile_enable(1)
        csma_batch()
        eng.sync()
        for name, v in eng.profile_kernels().items():
            if name.startswith("k_csma") or name.startswith("k_ccab"):
                per.setdefault(name, []).append(v[1] * 1e3 / max(v[0], 1))
        eng.profile_enable(0)
    out["kernels_us"] = {name: stats(v) for name, v in per.items()}
    out["kernels_us_sum_of_medians"] = float(sum(s["median_us"] for s in out["kernels_us"].values()))
    print(json.dumps(out))
    for d in dev + [d_f, d_e, d_st, d_at, d_tk, d_cst, d_cat, d_ctk]:
        d.free()
    eng.close()


if __name__ == "__main__":
    main()
