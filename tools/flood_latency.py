"""Latency of one dissemination step (rm_flood.hip) at the bench's 100 k node shape (the log-distance medium with
shadowing, BASELINE configs[2]'s field): one seed, then steps of  sources -> rm_tick_run_sources_device -> advance.  One process, two
contexts over the same table.

  device step         rm_flood_sources_device, rm_tick_run_sources_device with n = cap over the list where it lies,
                      rm_flood_advance_device; no host synchronisation inside the step, one rm_sync behind it: host clock around all
  kernels             the k_flood_* kernels' own dispatch intervals (rm_profile_kernels) summed per step, in steps of their own
  yardstick           the route that exists without the feature: the host keeps the Trickle state (HostFlood below: numpy, the rules of
                      DESIGN.md section 6, E20, for lone ungated ticks over lists that came from sources()), uploads the step's source
                      list, runs the tick, copies the whole result out (rm_result_copy) and advances its state from it

Before anything is timed both routes run `check` steps from the same state, then `grow` more so that the flood has a front worth
timing, and the device's whole table and totals are compared with the host's; again after the timed and the profiled steps.  Then
medians of `reps` consecutive steps after two warm-up steps, with min and max.  Prints one JSON line.
Run on the GPU box:  python tools/flood_latency.py [reps]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

M32 = np.uint64(0xFFFFFFFF)
FIELDS = ("first_us", "start_us", "fire_us", "rssi_bits", "parent", "hop", "interval", "c", "sent", "suppressed", "heard", "deferred")
TOTALS = ("covered", "seeds", "sent", "suppressed", "heard", "deferred", "stray", "skipped_slots", "max_hop", "last_first_us")
DELIVERED = 2


def mix64(z):
    z = z.astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def mulhi(a, b):
    """the high 64 bits of the 128-bit product of two uint64 arrays"""
    a0, a1, b0, b1 = a & M32, a >> np.uint64(32), b & M32, b >> np.uint64(32)
    w1 = a1 * b0 + ((a0 * b0) >> np.uint64(32))
    w2 = a0 * b1 + (w1 & M32)
    return a1 * b1 + (w1 >> np.uint64(32)) + (w2 >> np.uint64(32))


class HostFlood:
    """E20 on the host with numpy, for what the yardstick needs: seeds, source lists, and advances over lone ungated ticks whose
    lists came from sources() at the frames' start (no duplicates, no deferred candidate, one frame end per tick)"""

    def __init__(self, n, imin_us=8000, doublings=4, max_intervals=8, redundancy=2, max_hops=255, seed=0):
        self.n, self.imin, self.D, self.M, self.k, self.max_hops, self.seed = n, imin_us, doublings, max_intervals, redundancy, max_hops, seed
        self.a = {f: np.zeros(n, dtype=np.int64) for f in FIELDS}
        for f in ("first_us", "start_us", "fire_us", "parent", "hop"):
            self.a[f][:] = -1
        self.a["rssi_bits"] = np.zeros(n, dtype=np.uint64)
        self.t = {"seeds": 0, "stray": 0, "skipped_slots": 0}

    def _schedule(self, j):
        """interval a["interval"][j] of the nodes j (an index array)"""
        a = self.a
        m, first = a["interval"][j], a["first_us"][j]
        g = np.minimum(m, self.D)
        length = np.int64(self.imin) << g
        start = first + np.int64(self.imin) * ((np.int64(1) << g) - 1) + (m - g) * length
        half = (length >> 1).astype(np.uint64)
        h = mix64(mix64(mix64(np.array([(self.seed + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)) ^ (j.astype(np.uint64) & M32))
                  ^ first.astype(np.uint64))
        h = mix64(h ^ m.astype(np.uint64))
        done = m >= self.M
        a["start_us"][j] = np.where(done, -1, start)
        a["fire_us"][j] = np.where(done, -1, start + half.astype(np.int64) + mulhi(h, half).astype(np.int64))

    def _due(self, t):
        a = self.a
        return (a["first_us"] >= 0) & (a["interval"] < self.M) & (a["fire_us"] <= t)

    def seed_nodes(self, nodes, t):
        a = self.a
        j = np.unique(np.asarray(nodes, dtype=np.int64))
        j = j[(j >= 0) & (j < self.n)]
        j = j[a["first_us"][j] < 0]
        a["first_us"][j], a["parent"][j], a["hop"][j], a["interval"][j], a["c"][j], a["rssi_bits"][j] = t, -1, 0, 0, 0, 0
        self._schedule(j)
        self.t["seeds"] += len(j)

    def sources(self, t, cap):
        a = self.a
        due = self._due(t)
        supp = np.flatnonzero(due & (a["c"] >= self.k)) if self.k > 0 else np.zeros(0, dtype=np.int64)
        due[supp] = False
        a["suppressed"][supp] += 1
        a["interval"][supp] += 1
        a["c"][supp] = 0
        self._schedule(supp)
        s = np.flatnonzero(due)
        out = np.full(cap, -1, dtype=np.int32)
        out[:min(cap, len(s))] = s[:cap]
        return out, len(s)

    def advance(self, lst, pkt_offset, dst, verdict, rssi, start, air, lost=False):
        """lst: the tick's source list (padding -1); the rest: the tick's copied-out result"""
        if lost:
            self.t["skipped_slots"] += 1
            return
        a = self.a
        src = np.asarray(lst, dtype=np.int64)
        has = a["first_us"] >= 0
        inside = (src >= 0) & (src < self.n)
        cand = src[inside & has[np.clip(src, 0, self.n - 1)]]
        assert len(np.unique(cand)) == len(cand)
        due = self._due(start)[cand]
        self.t["stray"] += int((~due).sum())
        senders = cand[due]
        sending = np.zeros(self.n, dtype=bool)
        sending[senders] = True
        t_end = start + air
        off = np.asarray(pkt_offset, dtype=np.int64)
        n_links = int(off[-1])
        d = np.asarray(dst[:n_links], dtype=np.int64)
        s = src[np.repeat(np.arange(len(src)), np.diff(off))]
        ok = (np.asarray(verdict[:n_links]) == DELIVERED) & (s >= 0) & (s < self.n) & (d >= 0) & (d < self.n)
        ok &= has[np.clip(s, 0, self.n - 1)]
        np.add.at(a["heard"], d[ok], 1)
        hears = ok & has[d] & ~sending[d] & (t_end >= a["start_us"][d])
        new = np.flatnonzero(ok & ~has[d] & (a["hop"][np.clip(s, 0, self.n - 1)] + 1 <= self.max_hops))
        np.add.at(a["c"], d[hears], 1)
        a["sent"][senders] += 1
        a["interval"][senders] += 1
        a["c"][senders] = 0
        self._schedule(senders)
        # one frame end per tick: the least packet number wins, and the links lie in packet order
        w, at = np.unique(d[new], return_index=True)
        at = new[at]
        a["first_us"][w], a["parent"][w], a["hop"][w], a["interval"][w], a["c"][w] = t_end, s[at], a["hop"][s[at]] + 1, 0, 0
        a["rssi_bits"][w] = np.ascontiguousarray(rssi[:n_links], dtype=np.float64).view(np.uint64)[at]
        self._schedule(w)

    def totals(self):
        a = self.a
        has = a["first_us"] >= 0
        t = {f: int(a[f].sum()) for f in ("sent", "suppressed", "heard", "deferred")}
        t.update(covered=int(has.sum()), seeds=self.t["seeds"], stray=self.t["stray"], skipped_slots=self.t["skipped_slots"],
                 max_hop=int(a["hop"][has].max()) if has.any() else 0, last_first_us=int(a["first_us"][has].max()) if has.any() else 0)
        return t


def same(eng, host, what):
    """the device's whole table and totals against the host's"""
    rows, tot = eng.flood_read()
    for f in FIELDS:
        assert (rows[f].astype(host.a[f].dtype) == host.a[f]).all(), (what, f)
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
    n, cap, check, grow, warm = 100_000, 16384, 6, 60, 2
    tick, air, start_at = W.TICK_US, 640, 100
    params = dict(imin_us=2 * tick, doublings=3, max_intervals=64, redundancy=2, max_hops=255, seed=20)
    cfg = W.CONFIGS["c3"]
    nodes = W.make_nodes(n, cfg["index"])
    _, kw = W.model_kwargs(cfg["model"])
    engs = []
    for _ in range(2):      # [0] the device route, [1] the yardstick's ticks
        e = rsa.Engine(0)
        e.upload_table(nodes)
        e.set_model(rsa.MODEL_LOGDIST, **kw)
        e.set_link_capacity(1 << 22)
        engs.append(e)
    dev, yard = engs
    d_src, d_cnt, d_list = DeviceArray(nbytes=4 * cap), DeviceArray(nbytes=4), DeviceArray(nbytes=4 * cap)
    keep = [d_src, d_cnt, d_list]
    out = {"unit": "us per step; kernels: summed dispatch intervals of the k_flood_* kernels per step", "nodes": n, "cap": cap, "air_us": air,
           "tick_us": tick, "params": params}
    try:
        dev.flood_enable(**params)
        dev.flood_seed([n // 2], 0)
        host = HostFlood(n, **params)
        host.seed_nodes([n // 2], 0)
        same(dev, host, "after the seed")
        clock = [0]

        def device_step():
            t = clock[0]
            dev.flood_sources_device(t + start_at, cap, d_src.ptr.value, d_cnt.ptr.value)
            dev.tick_run_sources_device(t, t + tick, d_src.ptr.value, cap, t + start_at, air)
            dev.flood_advance_device(0, None, 0)
            dev.sync()

        def host_step():
            t = clock[0]
            lst, _ = host.sources(t + start_at, cap)
            assert d_list._hip.hipMemcpy(d_list.ptr, C.c_void_p(lst.ctypes.data), C.c_size_t(lst.nbytes), 1) == 0   # H2D
            yard.tick_run_sources_device(t, t + tick, d_list.ptr.value, cap, t + start_at, air)
            r = yard.result_copy(cap, cap=1 << 22)
            host.advance(lst, r.pkt_offset, r.dst, r.verdict, r.rssi, t + start_at, air)

        # 1. the two routes agree, step by step, before anything is timed; then the flood grows a front
        for k in range(check + grow):
            device_step()
            host_step()
            clock[0] += tick
            if k < check or k == check + grow - 1:
                same(dev, host, "check step %d" % k)
        out["checked_steps"], out["grown_steps"] = check, grow
        out["state_before_timing"] = host.totals()
        # 2. consecutive steps, both routes in lock step (so that the yardstick's state stays the device's)
        t_dev, t_host = [], []
        for k in range(reps + warm):
            t0 = time.perf_counter()
            device_step()
            t1 = time.perf_counter()
            host_step()
            t2 = time.perf_counter()
            clock[0] += tick
            if k >= warm:
                t_dev.append((t1 - t0) * 1e6)
                t_host.append((t2 - t1) * 1e6)
        same(dev, host, "after the timed steps")
        out["device_step"], out["yardstick_step"] = stats(t_dev), stats(t_host)
        out["state_after_timing"] = host.totals()
        # 3. the kernels' own dispatch intervals, in steps of their own
        per, launches = {}, {}
        for k in range(reps):
            dev.profile_enable(1)
            device_step()
            host_step()
            clock[0] += tick
            for name, v in dev.profile_kernels().items():
                if name.startswith("k_flood_"):
                    per.setdefault(name, []).append(v[1] * 1e3)
                    launches[name] = int(v[0])
            dev.profile_enable(0)
        out["kernels"] = {name: dict(stats(v), launches=launches[name]) for name, v in per.items()}
        out["kernels_sum_median_us"] = float(sum(np.median(v) for v in per.values()))
        same(dev, host, "after the profiled steps")
    finally:
        for d in keep:
            d.free()
        for e in engs:
            e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
