"""Latency of one link-estimator fold (rm_linkest.hip) at the bench's 100 k node shape (the log-distance medium with
shadowing, BASELINE configs[2]'s field), K = 8, over the context's own tables: the watch table filled by the neighbour tables from
beacon ticks, the forwarding queues driven along measured routes.  One process, one context.

  device fold   rm_linkest_fold_device(NULL) + rm_sync: host clock around both
  kernel        k_lest_fold's own dispatch interval (rm_profile_kernels), in folds of their own
  yardstick     the route that exists without the feature: rm_linkstats_peers_get, rm_linkstats_read and rm_fwd_read to the host,
                the rule in numpy (HostLinkEst below: DESIGN.md section 6, E23), and the published table copied to device memory
                for rm_etx_query_device's explicit tables

Between folds the tables move: a beacon tick of random senders with a neighbour-table update, and a forwarding tick with an advance.
Before anything is timed both routes run `check` folds from the same state and the device's entries, node state, published table
and totals are compared with the host's; again after the timed and the profiled folds.  Then medians of `reps` folds after two
warm-up folds, with min and max.  Prints one JSON line per table size and writes them to profiles/linkest_latency.json.
Run on the GPU box:  python tools/linkest_latency.py [reps] [--also-1m]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
U = np.uint64
LINK_STATS = np.dtype([("heard", "<u8"), ("delivered", "<u8"), ("rssi_q8_sum", "<i8"), ("sinr_q8_sum", "<i8"), ("first_start_us", "<i8"),
                       ("last_start_us", "<i8")])
ENTRY = np.dtype([("base_heard", "<u8"), ("base_delivered", "<u8"), ("etx", "<u4"), ("windows", "<u4"), ("data_windows", "<u4"), ("peer", "<i4")])
NODE = np.dtype([("base_tx", "<u8"), ("base_ack", "<u8"), ("base_next", "<i4"), ("data_samples", "<u4"), ("data_unmatched", "<u4"),
                 ("restarted", "<u4")])
TOTALS = ("folds", "beacon_samples", "data_samples", "data_unmatched", "restarted", "cleared", "estimates", "reserved")


class HostLinkEst:
    """E23 on the host with numpy: the entries, the node state, the published table and the totals"""

    def __init__(self, n, K, beacon_window=3, data_window=5, beacon_alpha_q8=230, data_alpha_q8=230, max_etx=6400):
        self.n, self.K = n, K
        self.bw, self.dw, self.ba, self.da, self.cap = beacon_window, data_window, beacon_alpha_q8, data_alpha_q8, max_etx
        self.bh, self.bd = np.zeros((n, K), dtype=U), np.zeros((n, K), dtype=U)
        self.etx, self.win, self.dwin = (np.zeros((n, K), dtype=U) for _ in range(3))
        self.peer = np.full((n, K), -1, dtype=np.int32)
        self.btx, self.back = np.zeros(n, dtype=U), np.zeros(n, dtype=U)
        self.bnext = np.full(n, -1, dtype=np.int32)
        self.samples, self.unmatched, self.restarted = (np.zeros(n, dtype=U) for _ in range(3))
        self.pub_peer = np.full((n, K), -1, dtype=np.int32)
        self.pub_stats = np.zeros((n, K), dtype=LINK_STATS)
        self.pub_stats["first_start_us"] = I64_MAX
        self.pub_stats["last_start_us"] = I64_MIN
        self.t = dict.fromkeys(TOTALS, 0)
        self.changed = 0          # entries whose published form changed in the last fold

    def _sample(self, dn, dd):
        with np.errstate(over="ignore"):
            q = np.maximum((U(128) * dn + (dd >> U(1))) // np.maximum(dd, U(1)), U(128))
        return np.where(dd == 0, U(self.cap), np.minimum(q, U(self.cap)))

    @staticmethod
    def _ewma(a, old, s):
        return np.where(old == 0, s, (U(a) * old + U(256 - a) * s + U(128)) >> U(8))

    def fold(self, peer, heard, delivered, fwd=None):
        """peer int32 [n][K], heard and delivered uint64 [n][K], fwd: None or (next int32 [n], acked uint64 [n], failed uint64 [n])"""
        n = self.n
        rows = np.arange(n)
        q = peer.astype(np.int64)
        H, D = heard.astype(U), delivered.astype(U)
        etx0, peer0 = self.etx.copy(), self.peer.copy()
        empty = (q < 0) | (q >= n) | (q == rows[:, None])
        cleared = empty & (self.peer != -1)
        restart = ~empty & ((peer != self.peer) | (H < self.bh) | (D < self.bd))
        anew = empty | restart
        for a in (self.bh, self.bd, self.etx, self.win, self.dwin):
            a[anew] = 0
        self.peer = np.where(empty, -1, peer).astype(np.int32)
        self.restarted += restart.sum(axis=1).astype(U)
        with np.errstate(over="ignore"):
            dH, dD = H - self.bh, D - self.bd
        samp = ~empty & (self.bw > 0) & (dH >= U(self.bw))
        new = self._ewma(self.ba, self.etx, self._sample(dH, dD))
        self.etx[samp] = new[samp]
        self.win[samp] += U(1)
        self.bh[samp], self.bd[samp] = H[samp], D[samp]
        t = self.t
        t["folds"] += 1
        t["beacon_samples"] += int(samp.sum())
        t["restarted"] += int(restart.sum())
        t["cleared"] += int(cleared.sum())
        if fwd is not None and self.dw > 0:
            w = np.asarray(fwd[0]).astype(np.int64)
            A = np.asarray(fwd[1]).astype(U)
            with np.errstate(over="ignore"):
                T = A + np.asarray(fwd[2]).astype(U)
                dT, dA = T - self.btx, A - self.back
            rebase = (w != self.bnext) | (T < self.btx) | (A < self.back)
            due = ~rebase & (w >= 0) & (w < n) & (w != rows) & (dT >= U(self.dw))
            move = rebase | due
            self.btx[move], self.back[move] = T[move], A[move]
            self.bnext[rebase] = w[rebase]
            match = (self.peer == w[:, None]) & due[:, None]
            has = match.any(axis=1)
            r = np.flatnonzero(has)
            k = match[r].argmax(axis=1)
            self.etx[r, k] = self._ewma(self.da, self.etx[r, k], self._sample(dT[r], dA[r]))
            self.dwin[r, k] += U(1)
            self.samples[r] += U(1)
            unm = due & ~has
            self.unmatched[unm] += U(1)
            t["data_samples"] += len(r)
            t["data_unmatched"] += int(unm.sum())
        t["estimates"] = int((self.etx != 0).sum())
        ch = (self.etx != etx0) | (self.peer != peer0)
        self.changed = int(ch.sum())
        self.pub_peer[ch] = self.peer[ch]
        self.pub_stats["heard"][ch] = self.etx[ch]
        self.pub_stats["delivered"][ch] = np.where(self.etx[ch] != 0, U(128), U(0))

    def entries(self):
        e = np.zeros((self.n, self.K), dtype=ENTRY)
        for f, a in (("base_heard", self.bh), ("base_delivered", self.bd), ("etx", self.etx), ("windows", self.win), ("data_windows", self.dwin),
                     ("peer", self.peer)):
            e[f] = a
        return e

    def nodes(self):
        e = np.zeros(self.n, dtype=NODE)
        for f, a in (("base_tx", self.btx), ("base_ack", self.back), ("base_next", self.bnext), ("data_samples", self.samples),
                     ("data_unmatched", self.unmatched), ("restarted", self.restarted)):
            e[f] = a
        return e

    def totals(self):
        return dict(self.t)


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def run(n, reps):
    import radio_sim_amd as rsa
    from radio_sim_amd import workload as W
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from util import DeviceArray

    K, cap, check, warm, fill = 8, 4096, 3, 2, 24
    tick, air, start_at = W.TICK_US, 640, 100
    params = dict(beacon_window=3, data_window=5, beacon_alpha_q8=230, data_alpha_q8=230, max_etx=6400)
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    eng = rsa.Engine(0)
    rng = np.random.default_rng(23)
    d_list = DeviceArray(nbytes=4 * cap)
    d_src, d_count = DeviceArray(nbytes=4 * cap), DeviceArray(nbytes=4)
    d_pub_peer, d_pub_stats = DeviceArray(nbytes=4 * n * K), DeviceArray(nbytes=48 * n * K)
    hip = d_list._hip
    out = {"unit": "us per fold; kernel: k_lest_fold's own dispatch interval", "nodes": n, "K": K, "senders_per_tick": cap, "params": params}
    try:
        eng.upload_table(nodes)
        eng.set_model(rsa.MODEL_LOGDIST, **kw)
        eng.set_link_capacity(1 << 22)
        eng.linkstats_enable(K)
        eng.nbtable_enable(admit_rssi_dbm=-92.0, timeout_us=0, evict_cost=0)
        clock = [0]

        def beacon_tick():
            t = clock[0]
            lst = np.sort(rng.choice(n, cap, replace=False)).astype(np.int32)
            assert hip.hipMemcpy(d_list.ptr, C.c_void_p(lst.ctypes.data), C.c_size_t(lst.nbytes), 1) == 0   # H2D
            eng.tick_run_sources_device(t, t + tick, d_list.ptr.value, cap, t + start_at, air)
            eng.nbtable_update_device(0, t + tick, None)
            clock[0] += tick

        def fwd_tick():
            t = clock[0]
            eng.fwd_inject_device(d_list.ptr.value, cap, t)
            eng.fwd_sources_device(t + start_at, cap, d_src.ptr.value, d_count.ptr.value)
            eng.tick_run_sources_device(t, t + tick, d_src.ptr.value, cap, t + start_at, air)
            eng.fwd_advance_device(0, None, 0)
            clock[0] += tick
        for _ in range(fill):
            beacon_tick()
        # routes over the raw counters toward 64 roots, then the forwarding queues along them
        roots = np.sort(rng.choice(n, 64, replace=False)).astype(np.int32)
        routes, rt = eng.etx_routes(eng.etx_params(min_heard=1), roots)
        eng.fwd_enable(queue_slots=4)
        eng.fwd_set_next(routes["parent"], roots, clock[0])
        out["routes_reached"] = rt["reached"]
        eng.linkest_enable(K, **params)
        host = HostLinkEst(n, K, **params)
        parts = {k: [] for k in ("device_fold", "read", "rule", "upload", "changed_entries")}

        def same(what):
            ent, nod, tot = eng.linkest_read()
            pp, ps, _ = eng.linkest_tables()
            assert ent.tobytes() == host.entries().tobytes(), (what, "entries")
            assert nod.tobytes() == host.nodes().tobytes(), (what, "node state")
            assert DeviceArray.read(pp, np.int32, n * K).tobytes() == host.pub_peer.tobytes(), (what, "published peers")
            assert DeviceArray.read(ps, LINK_STATS, n * K).tobytes() == host.pub_stats.tobytes(), (what, "published entries")
            assert tot == host.totals(), (what, tot, host.totals())

        def step(timed):
            for _ in range(3):
                beacon_tick()
                fwd_tick()
            eng.sync()
            t0 = time.perf_counter()
            eng.linkest_fold_device(None)
            eng.sync()
            t1 = time.perf_counter()
            peer = eng.linkstats_peers()
            st = eng.linkstats_read()[0]
            fw = eng.fwd_read()[0]
            t2 = time.perf_counter()
            host.fold(peer, st["heard"], st["delivered"], (fw["next"], fw["acked"], fw["failed"]))
            t3 = time.perf_counter()
            assert hip.hipMemcpy(d_pub_peer.ptr, C.c_void_p(host.pub_peer.ctypes.data), C.c_size_t(host.pub_peer.nbytes), 1) == 0
            assert hip.hipMemcpy(d_pub_stats.ptr, C.c_void_p(host.pub_stats.ctypes.data), C.c_size_t(host.pub_stats.nbytes), 1) == 0
            t4 = time.perf_counter()
            if timed:
                for name, a, b in (("device_fold", t0, t1), ("read", t1, t2), ("rule", t2, t3), ("upload", t3, t4)):
                    parts[name].append((b - a) * 1e6)
                parts["changed_entries"].append(host.changed)
        # 1. the two routes agree, fold by fold, before anything is timed
        for k in range(check):
            step(False)
            same("check fold %d" % k)
        out["checked_folds"] = check
        # 2. consecutive folds
        for k in range(warm):
            step(False)
        for k in range(reps):
            step(True)
        same("after the timed folds")
        for name in ("device_fold", "read", "rule", "upload"):
            out[name] = stats(parts[name])
        out["yardstick_fold"] = {"median_us": out["read"]["median_us"] + out["rule"]["median_us"] + out["upload"]["median_us"],
                                 "what": "read + rule + upload medians"}
        out["changed_entries_median"] = float(np.median(parts["changed_entries"]))
        # 3. the kernel's own dispatch interval, in folds of their own
        per, launches = [], 0
        for k in range(reps):
            for _ in range(3):
                beacon_tick()
                fwd_tick()
            eng.sync()
            eng.profile_enable(1)
            eng.linkest_fold_device(None)
            eng.sync()
            for name, v in eng.profile_kernels().items():
                if name.startswith("k_lest_fold"):
                    per.append(v[1] * 1e3 / max(int(v[0]), 1))
                    launches = int(v[0])
            eng.profile_enable(0)
            peer, st, fw = eng.linkstats_peers(), eng.linkstats_read()[0], eng.fwd_read()[0]
            host.fold(peer, st["heard"], st["delivered"], (fw["next"], fw["acked"], fw["failed"]))
        same("after the profiled folds")
        out["kernel"] = dict(stats(per), launches_per_fold=launches)
        bound = n * K * (48 + 84)
        moved = n * K * (4 + 16 + 32) + n * (32 + 20) + int(out["changed_entries_median"]) * (32 + 4 + 48)
        out["bytes"] = {"bound_n_K_132": bound, "estimate_moved": moved,
                        "what": "estimate: 52 bytes read per entry and 52 per node, 84 written per entry whose published form changed (median)",
                        "bound_GBps_at_kernel_median": bound / out["kernel"]["median_us"] / 1e3,
                        "estimate_GBps_at_kernel_median": moved / out["kernel"]["median_us"] / 1e3}
        out["state_after"] = host.totals()
    finally:
        for d in (d_list, d_src, d_count, d_pub_peer, d_pub_stats):
            d.free()
        eng.close()
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0]) if args else 10)
    sizes = [100_000] + ([1_000_000] if "--also-1m" in sys.argv else [])
    results = []
    for n in sizes:
        r = run(n, reps)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(os.path.join(ROOT, "profiles", "linkest_latency.json"), "w") as f:
            f.write(json.dumps(results if len(results) > 1 else results[0]) + "\n")


if __name__ == "__main__":
    main()
