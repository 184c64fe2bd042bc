"""Latency of one neighbour-table step and of the expire walk (rm_nbtable.hip) at the bench's 100 k node shape (the
log-distance medium with shadowing, BASELINE configs[2]'s field), K = 8, from an empty watch table: steps of
rm_tick_run_sources_device -> update.  One process, two contexts over the same table.

  device step         rm_tick_run_sources_device over a list of beacon senders where it lies, rm_nbtable_update_device; no host
                      synchronisation inside the step, one rm_sync behind it: host clock around all
  device update       the same with the host clock around the update and its rm_sync alone (the tick waited for first)
  kernels             the k_nbt_* kernels' own dispatch intervals (rm_profile_kernels) summed per step, in steps of their own
  yardstick           the route that exists without the feature: the slot's result copied to the host (rm_result_copy), the rule in
                      numpy (HostNbTable below: DESIGN.md section 6, E22) and rm_linkstats_watch of the changed rows.  The host keeps
                      the counters it judges by from the copied results (its own E14 pass, timed apart as "host_count"): a watch
                      clears an entry, so the engine's counters cannot hold step 3's links
  expire              rm_nbtable_expire_device + rm_sync against the numpy walk + rm_linkstats_watch of the changed rows

Before anything is timed both routes run `check` steps from the same state and the device's peers, entries, counters and totals are
compared with the host's; again after the timed and the profiled steps.  Then medians of `reps` consecutive steps after two warm-up
steps, with min and max.  Prints one JSON line.
Run on the GPU box:  python tools/nbtable_latency.py [reps]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

DELIVERED = 2
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
COLS = ("heard", "delivered", "rssi_q8_sum", "sinr_q8_sum", "first_start_us", "last_start_us")
NODE_FIELDS = ("admitted", "evicted_stale", "evicted_poor", "refused", "expired")


def q8(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.fabs(x) < 2147483648.0
        v = np.floor(np.where(ok, x, 0.0) * 256.0 + 0.5)
    return np.where(ok, v, 0.0).astype(np.int64)


class HostNbTable:
    """E22 (and E14's pass) on the host with numpy: the tables, the counters and the totals"""

    def __init__(self, n, K, admit_rssi_dbm=-95.0, timeout_us=60_000_000, min_heard=4, evict_cost=1024, require_delivered=1):
        self.n, self.K = n, K
        self.admit, self.timeout, self.min_heard, self.evict_cost, self.req = admit_rssi_dbm, timeout_us, min_heard, evict_cost, require_delivered
        self.peer = np.full((n, K), -1, dtype=np.int32)
        self.s = {c: np.zeros((n, K), dtype=np.uint64 if c in ("heard", "delivered") else np.int64) for c in COLS}
        self.s["first_start_us"][...] = I64_MAX
        self.s["last_start_us"][...] = I64_MIN
        self.cnt = {f: np.zeros(n, dtype=np.int64) for f in NODE_FIELDS}
        self.t = {"updates": 0, "skipped_slots": 0}

    def _links(self, src, start, off, dst):
        """per link: source, start, receiver, and whether both ends are in the table"""
        off = np.asarray(off, dtype=np.int64)
        L = int(off[-1])
        p = np.repeat(np.arange(len(src)), np.diff(off))
        s, d = np.asarray(src, dtype=np.int64)[p], np.asarray(dst[:L], dtype=np.int64)
        ok = (s >= 0) & (s < self.n) & (d >= 0) & (d < self.n)
        return L, s, np.asarray(start, dtype=np.int64)[p], d, ok

    def _add(self, d, k, verdict, rssi, sinr, start):
        s = self.s
        np.add.at(s["heard"], (d, k), np.uint64(1))
        np.add.at(s["delivered"], (d, k), (verdict == DELIVERED).astype(np.uint64))
        np.add.at(s["rssi_q8_sum"], (d, k), q8(rssi))
        if sinr is not None:
            np.add.at(s["sinr_q8_sum"], (d, k), q8(sinr))
        np.minimum.at(s["first_start_us"], (d, k), start)
        np.maximum.at(s["last_start_us"], (d, k), start)

    def count(self, src, start, off, dst, verdict, rssi, sinr=None):
        """E14's pass over one finished tick"""
        L, s, st, d, ok = self._links(src, start, off, dst)
        if L == 0:
            return
        hit = (self.peer[np.where(ok, d, 0)] == s[:, None]) & ok[:, None]
        m = hit.any(axis=1)
        k = self.K - 1 - hit[m][:, ::-1].argmax(axis=1)      # (the pass keeps the last matching slot; valid peers are distinct)
        self._add(d[m], k, np.asarray(verdict[:L])[m], np.asarray(rssi[:L])[m], None if sinr is None else np.asarray(sinr[:L])[m], st[m])

    def _pinned(self, rows, pin):
        """[len(rows)][K]: the slot holds the row's pinned peer"""
        if pin is None:
            return np.zeros((len(rows), self.K), dtype=bool)
        pn = np.asarray(pin, dtype=np.int64)[rows]
        return ((pn >= 0) & (pn < self.n))[:, None] & (self.peer[rows] == pn[:, None])

    def _stale(self, rows, t):
        last = self.s["last_start_us"][rows]
        if self.timeout <= 0:
            return np.zeros(last.shape, dtype=bool)
        old = last < t - self.timeout if t >= self.timeout else np.zeros(last.shape, dtype=bool)
        return (last == I64_MIN) | old

    def update(self, src, start, off, dst, verdict, rssi, time_us, sinr=None, pin=None, lost=False):
        """-> the nodes whose rows changed"""
        if lost:
            self.t["skipped_slots"] += 1
            return np.zeros(0, dtype=np.int64)
        self.t["updates"] += 1
        n, K = self.n, self.K
        L, s, st, d, ok = self._links(src, start, off, dst)
        if L == 0:
            return np.zeros(0, dtype=np.int64)
        verdict, rssi = np.asarray(verdict[:L]), np.asarray(rssi[:L], dtype=np.float64)
        held = (self.peer[np.where(ok, d, 0)] == s[:, None]).any(axis=1)
        with np.errstate(invalid="ignore"):
            bids = ok & (s != d) & ~held & (rssi >= self.admit)
        if self.req:
            bids &= verdict == DELIVERED
        qc = np.clip(q8(rssi), -(1 << 30), 1 << 30)
        key = ((qc + (1 << 30) + 1).astype(np.uint64) << np.uint64(32)) | (0x7FFFFFFF - s).astype(np.uint64)
        best = np.zeros(n, dtype=np.uint64)
        np.maximum.at(best, d[bids], key[bids])
        rows = np.flatnonzero(best)
        if len(rows) == 0:
            return rows
        win = 0x7FFFFFFF - (best[rows] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        pr = self.peer[rows].astype(np.int64)
        empty = (pr < 0) | (pr >= n) | (pr == rows[:, None])
        free = ~self._pinned(rows, pin)
        last = self.s["last_start_us"][rows]
        stale = free & self._stale(rows, time_us)
        H, D = self.s["heard"][rows], self.s["delivered"][rows]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(D == 0, U64_MAX, np.maximum((np.uint64(128) * H + (D >> np.uint64(1))) // np.maximum(D, np.uint64(1)), np.uint64(128)))
        poor = free & (self.evict_cost > 0) & (H >= np.uint64(max(self.min_heard, 1))) & (c > np.uint64(self.evict_cost))
        slot = np.full(len(rows), -1, dtype=np.int64)
        kind = np.zeros(len(rows), dtype=np.int64)
        has = empty.any(axis=1)
        slot[has] = empty[has].argmax(axis=1)
        m = (slot < 0) & stale.any(axis=1)
        slot[m] = np.where(stale[m], last[m], I64_MAX).argmin(axis=1)        # (the least last_start_us, then the least k)
        # (a stale slot whose last_start_us is INT64_MAX ties with the mask's filler; argmin still returns the first of them, and a
        # filler in front of it would be a slot that is not stale -- settle by the mask)
        bad = m.copy()
        bad[m] = ~stale[m, slot[m]]
        for r in np.flatnonzero(bad):
            slot[r] = np.flatnonzero(stale[r])[0]
        kind[m] = 1
        m = (slot < 0) & poor.any(axis=1)
        slot[m] = np.where(poor[m], c[m], np.uint64(0)).argmax(axis=1)       # (the greatest c_in, delivered == 0 above all; then the least k)
        kind[m] = 2
        ref = slot < 0
        self.cnt["refused"][rows[ref]] += 1
        rows, slot, kind, win = rows[~ref], slot[~ref], kind[~ref], win[~ref]
        self.peer[rows, slot] = win
        for col in COLS:
            self.s[col][rows, slot] = I64_MAX if col == "first_start_us" else I64_MIN if col == "last_start_us" else 0
        self.cnt["admitted"][rows] += 1
        self.cnt["evicted_stale"][rows[kind == 1]] += 1
        self.cnt["evicted_poor"][rows[kind == 2]] += 1
        # (3) the admitted peers' links of this slot
        got = np.full(n, -1, dtype=np.int64)
        at = np.zeros(n, dtype=np.int64)
        got[rows], at[rows] = win, slot
        m = ok & (got[np.where(ok, d, 0)] == s)
        self._add(d[m], at[d[m]], verdict[m], rssi[m], None if sinr is None else np.asarray(sinr[:L])[m], st[m])
        return rows

    def expire(self, time_us, pin=None):
        """-> the nodes whose rows changed"""
        rows = np.arange(self.n)
        pr = self.peer.astype(np.int64)
        goes = ~((pr < 0) | (pr >= self.n) | (pr == rows[:, None])) & ~self._pinned(rows, pin) & self._stale(rows, time_us)
        self.peer[goes] = -1
        for col in COLS:
            self.s[col][goes] = I64_MAX if col == "first_start_us" else I64_MIN if col == "last_start_us" else 0
        self.cnt["expired"] += goes.sum(axis=1)
        return np.flatnonzero(goes.any(axis=1))

    def totals(self):
        t = {f: int(self.cnt[f].sum()) for f in NODE_FIELDS}
        t.update(self.t, reserved=0)
        return t


def same(eng, host, what):
    """the device's peers, entries, counters and totals against the host's"""
    assert (eng.linkstats_peers() == host.peer).all(), (what, "peer")
    stats = eng.linkstats_read()[0]
    for c in COLS:
        assert (stats[c] == host.s[c]).all(), (what, c)
    rows, tot = eng.nbtable_read()
    for f in NODE_FIELDS:
        assert (rows[f].astype(np.int64) == host.cnt[f]).all(), (what, f)
    assert tot == host.totals(), (what, tot, host.totals())


def stats(us):
    us = np.sort(np.asarray(us, dtype=np.float64))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "max_us": float(us[-1]), "reps": len(us)}


def main():
    import radio_sim_amd as rsa
    from radio_sim_amd import workload as W
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from util import DeviceArray

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = max(5, int(args[0]) if args else 10)
    n, K, cap, check, warm = 100_000, 8, 4096, 4, 2
    tick, air, start_at = W.TICK_US, 640, 100
    params = dict(admit_rssi_dbm=-92.0, timeout_us=6 * tick, min_heard=2, evict_cost=512, require_delivered=1)
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    engs = []
    for _ in range(2):      # [0] the device route, [1] the yardstick's ticks and watch calls
        e = rsa.Engine(0)
        e.upload_table(nodes)
        e.set_model(rsa.MODEL_LOGDIST, **kw)
        e.set_link_capacity(1 << 22)
        e.linkstats_enable(K)
        engs.append(e)
    dev, yard = engs
    rng = np.random.default_rng(22)
    d_list = DeviceArray(nbytes=4 * cap)
    out = {"unit": "us per step; kernels: summed dispatch intervals of the k_nbt_* kernels per step", "nodes": n, "K": K, "senders_per_tick": cap,
           "air_us": air, "tick_us": tick, "params": params}
    try:
        dev.nbtable_enable(**params)
        host = HostNbTable(n, K, **params)
        clock = [0]
        parts = {k: [] for k in ("device_step", "device_update", "copy", "rule", "host_count", "watch", "links", "changed_rows")}

        def step(timed):
            t = clock[0]
            lst = np.sort(rng.choice(n, cap, replace=False)).astype(np.int32)
            assert d_list._hip.hipMemcpy(d_list.ptr, C.c_void_p(lst.ctypes.data), C.c_size_t(lst.nbytes), 1) == 0   # H2D
            t0 = time.perf_counter()
            dev.tick_run_sources_device(t, t + tick, d_list.ptr.value, cap, t + start_at, air)
            if timed == "update":
                dev.sync()
            t1 = time.perf_counter()
            dev.nbtable_update_device(0, t + tick, None)
            dev.sync()
            t2 = time.perf_counter()
            yard.tick_run_sources_device(t, t + tick, d_list.ptr.value, cap, t + start_at, air)
            yard.sync()
            t3 = time.perf_counter()
            r = yard.result_copy(cap, cap=1 << 22)
            t4 = time.perf_counter()
            start = np.full(cap, t + start_at, dtype=np.int64)
            host.count(lst, start, r.pkt_offset, r.dst, r.verdict, r.rssi)
            t5 = time.perf_counter()
            rows = host.update(lst, start, r.pkt_offset, r.dst, r.verdict, r.rssi, t + tick)
            t6 = time.perf_counter()
            if len(rows):
                yard.linkstats_watch(host.peer[rows], nodes=rows.astype(np.int32))
            yard.sync()
            t7 = time.perf_counter()
            clock[0] += tick
            if timed:
                parts["device_update" if timed == "update" else "device_step"].append((t2 - (t1 if timed == "update" else t0)) * 1e6)
                for name, a, b in (("copy", t3, t4), ("host_count", t4, t5), ("rule", t5, t6), ("watch", t6, t7)):
                    parts[name].append((b - a) * 1e6)
                parts["links"].append(int(r.count))
                parts["changed_rows"].append(len(rows))

        # 1. the two routes agree, step by step, before anything is timed
        for k in range(check):
            step(None)
            same(dev, host, "check step %d" % k)
        out["checked_steps"] = check
        out["state_before_timing"] = host.totals()
        # 2. consecutive steps
        for k in range(warm):
            step(None)
        for k in range(reps):
            step("step")
        for k in range(reps):
            step("update")
        same(dev, host, "after the timed steps")
        for name in ("device_step", "device_update", "copy", "rule", "host_count", "watch"):
            out[name] = stats(parts[name])
        out["yardstick_update"] = {"median_us": out["copy"]["median_us"] + out["rule"]["median_us"] + out["watch"]["median_us"],
                                   "what": "copy + rule + watch medians"}
        out["links_per_tick_median"] = float(np.median(parts["links"]))
        out["changed_rows_median"] = float(np.median(parts["changed_rows"]))
        out["state_after_timing"] = host.totals()
        # 3. the kernels' own dispatch intervals, in steps of their own
        per, launches = {}, {}
        for k in range(reps):
            dev.profile_enable(1)
            step(None)
            for name, v in dev.profile_kernels().items():
                if name.startswith("k_nbt_"):
                    per.setdefault(name, []).append(v[1] * 1e3)
                    launches[name] = int(v[0])
            dev.profile_enable(0)
        out["kernels"] = {name: dict(stats(v), launches=launches[name]) for name, v in per.items()}
        out["kernels_sum_median_us"] = float(sum(np.median(v) for v in per.values()))
        # 4. the expire walk: time passes, then every slot is stale
        t_dev, t_host, t_watch = [], [], []
        for k in range(reps):
            step(None)
            t = clock[0] + 20 * tick
            t0 = time.perf_counter()
            dev.nbtable_expire_device(t, None)
            dev.sync()
            t1 = time.perf_counter()
            rows = host.expire(t)
            t2 = time.perf_counter()
            if len(rows):
                yard.linkstats_watch(host.peer[rows], nodes=rows.astype(np.int32))
            yard.sync()
            t3 = time.perf_counter()
            t_dev.append((t1 - t0) * 1e6)
            t_host.append((t2 - t1) * 1e6)
            t_watch.append((t3 - t2) * 1e6)
        same(dev, host, "after the expire walks")
        out["expire_device"], out["expire_rule"], out["expire_watch"] = stats(t_dev), stats(t_host), stats(t_watch)
    finally:
        d_list.free()
        for e in engs:
            e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
