"""Latency of one forwarding step (rm_fwd.hip) at the bench's 100 k node shape (the log-distance medium with
shadowing, BASELINE configs[2]'s field): next hops from the hop query toward node 0, one packet injected at every tenth node, then
steps of  sources -> rm_tick_run_sources_device -> advance.  One process, two contexts over the same table.

  device step         rm_fwd_sources_device, rm_tick_run_sources_device with n = cap over the list where it lies, rm_fwd_advance_device;
                      no host synchronisation inside the step, one rm_sync behind it: host clock around all four
  kernels             the k_fwd_* kernels' own dispatch intervals (rm_profile_kernels) summed per step, in steps of their own
  yardstick           the route that exists without the feature: the host keeps the queues (HostQueues below: numpy, the rules of
                      DESIGN.md section 6, E19, for lists without duplicates), uploads the step's source list, runs the tick,
                      asks rm_unicast_query (host form) whether each frame reached next[src], and advances its queues

Before anything is timed both routes run the same `check` steps from the same state and the device's whole table, totals and
queues are compared with the host's.  Then medians of `reps` consecutive steps after two warm-up steps, with min and max.
Prints one JSON line.
Run on the GPU box:  python tools/fwd_latency.py [reps]
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
BIG = np.int64(1) << np.int64(62)
SINK, NO_ROUTE = -2, -1
COUNTERS = ("generated", "arrived", "lost", "latency_us_sum", "latency_us_max", "hops_sum", "attempts", "acked", "failed", "deferred",
            "rejected", "dropped")
TOTALS = ("generated", "arrived", "dropped_retries", "dropped_no_route", "dropped_full", "dropped_ttl", "in_flight", "stray", "skipped_slots",
          "latency_us_sum", "hops_sum")


def mix64(z):
    z = z.astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


class HostQueues:
    """E19 on the host with numpy, for what the yardstick needs: routes set once, injects, source lists, and advances over lists
    WITHOUT duplicates whose entries all came from sources() at the frames' start (so no stray, no deferred attempt)"""

    def __init__(self, n, queue_slots=8, max_retries=3, min_be=3, max_be=5, max_hops=64, backoff_unit_us=320, seed=0):
        self.n, self.Q = n, queue_slots
        self.max_retries, self.min_be, self.max_be, self.max_hops, self.unit, self.seed = max_retries, min_be, max_be, max_hops, backoff_unit_us, seed
        self.valid = np.zeros((n, queue_slots), dtype=bool)
        self.enq = np.zeros((n, queue_slots), dtype=np.int64)
        self.birth = np.zeros((n, queue_slots), dtype=np.int64)
        self.origin = np.zeros((n, queue_slots), dtype=np.int32)
        self.hops = np.zeros((n, queue_slots), dtype=np.int32)
        self.next = np.full(n, NO_ROUTE, dtype=np.int32)
        self.tries = np.zeros(n, dtype=np.int32)
        self.ready = np.zeros(n, dtype=np.int64)
        self.queue_max = np.zeros(n, dtype=np.int32)
        self.c = {f: np.zeros(n, dtype=np.uint64) for f in COUNTERS}
        self.t = {f: 0 for f in TOTALS}

    def set_next(self, parent, roots):
        """(before anything is queued: nothing to settle)"""
        assert not self.valid.any()
        p = np.asarray(parent, dtype=np.int64)
        j = np.arange(self.n)
        self.next[:] = np.where((p >= 0) & (p < self.n) & (p != j), p, NO_ROUTE)
        self.next[np.asarray(roots, dtype=np.int64)] = SINK

    def inject(self, src, t):
        """distinct nodes"""
        src = np.asarray(src, dtype=np.int64)
        assert len(np.unique(src)) == len(src)
        self.c["generated"][src] += np.uint64(1)
        self.t["generated"] += len(src)
        nx = self.next[src]
        sink, lost = src[nx == SINK], src[nx == NO_ROUTE]
        self.c["arrived"][sink] += np.uint64(1)
        self.t["arrived"] += len(sink)
        self.c["lost"][lost] += np.uint64(1)
        self.c["dropped"][lost] += np.uint64(1)
        self.t["dropped_no_route"] += len(lost)
        q = src[nx >= 0]
        full = self.valid[q].all(axis=1)
        self.c["lost"][q[full]] += np.uint64(1)
        self.c["dropped"][q[full]] += np.uint64(1)
        self.t["dropped_full"] += int(full.sum())
        q = q[~full]
        slot = np.argmin(self.valid[q], axis=1)      # the first free slot
        self.valid[q, slot] = True
        self.enq[q, slot], self.birth[q, slot], self.origin[q, slot], self.hops[q, slot] = t, t, q, 0
        self.queue_max[q] = np.maximum(self.queue_max[q], self.valid[q].sum(axis=1))
        self.t["in_flight"] += len(q)

    def sources(self, t, cap):
        head = np.where(self.valid, self.enq, BIG).min(axis=1)
        s = np.flatnonzero(self.valid.any(axis=1) & (self.ready <= t) & (head <= t))
        out = np.full(cap, -1, dtype=np.int32)
        out[:min(cap, len(s))] = s[:cap]
        return out, len(s)

    def _heads(self, rows):
        keys = (self.hops[rows], self.origin[rows], self.birth[rows], np.where(self.valid[rows], self.enq[rows], BIG))
        return np.lexsort(keys, axis=-1)[:, 0]

    def advance(self, lst, delivered, start, air):
        """lst: the tick's source list (padding -1); delivered[p]: rm_unicast_query's status of (p, next[lst[p]]) is DELIVERED"""
        lst = np.asarray(lst, dtype=np.int64)
        ok = lst >= 0
        S, D = lst[ok], np.asarray(delivered, dtype=bool)[ok]
        if len(S) == 0:
            return
        t_end = start + air
        head = self._heads(S)
        w = self.next[S].astype(np.int64)
        assert (w >= 0).all()
        self.c["attempts"][S] += np.uint64(1)
        sinkw = self.next[w] == SINK
        relay = D & ~sinkw
        length = self.valid.sum(axis=1)
        A = np.bincount(w[relay], minlength=self.n)
        accept = length[w] + A[w] <= self.Q
        acked = D & (sinkw | accept)
        np.add.at(self.c["rejected"], w[relay & ~accept], np.uint64(1))
        o, h, b = self.origin[S, head].astype(np.int64), self.hops[S, head], self.birth[S, head]
        # acked at a sink
        k = acked & sinkw
        lat = (t_end - b[k]).astype(np.uint64)
        np.add.at(self.c["arrived"], o[k], np.uint64(1))
        np.add.at(self.c["latency_us_sum"], o[k], lat)
        np.maximum.at(self.c["latency_us_max"], o[k], lat)
        np.add.at(self.c["hops_sum"], o[k], (h[k] + 1).astype(np.uint64))
        self.t["arrived"] += int(k.sum())
        self.t["latency_us_sum"] += int(lat.sum())
        self.t["hops_sum"] += int((h[k] + 1).sum())
        # acked at a relay: beyond max_hops dropped there, else pushed into the k-th slot free at the start
        r = acked & ~sinkw
        ttl = r & (h + 1 > self.max_hops)
        np.add.at(self.c["lost"], o[ttl], np.uint64(1))
        np.add.at(self.c["dropped"], w[ttl], np.uint64(1))
        self.t["dropped_ttl"] += int(ttl.sum())
        push = np.flatnonzero(r & ~ttl)
        push = push[np.argsort(w[push], kind="stable")]
        wp = w[push]
        first = np.searchsorted(wp, wp, side="left")
        rank = np.arange(len(wp)) - first
        slot = np.argsort(self.valid[wp], axis=1, kind="stable")[np.arange(len(wp)), rank]
        pushed = (wp, slot, t_end, b[push], o[push], h[push] + 1)
        np.maximum.at(self.queue_max, wp, (length[wp] + rank + 1).astype(np.int32))
        # failed
        f = ~acked
        self.c["failed"][S[f]] += np.uint64(1)
        tries = self.tries[S] + 1
        gone = f & (tries > self.max_retries)
        np.add.at(self.c["lost"], o[gone], np.uint64(1))
        self.c["dropped"][S[gone]] += np.uint64(1)
        self.t["dropped_retries"] += int(gone.sum())
        wait = f & ~gone
        be = np.minimum(self.min_be + tries[wait] - 1, self.max_be)
        h1 = mix64(mix64(mix64(np.array([(self.seed + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)) ^ S[wait].astype(np.uint64))
                   ^ np.uint64(start))
        h2 = mix64(h1 ^ tries[wait].astype(np.uint64))
        rr = np.where(be > 0, h2 >> (np.uint64(64) - np.maximum(be, 1).astype(np.uint64)), np.uint64(0)).astype(np.int64)
        self.tries[S[wait]] = tries[wait]
        self.ready[S[wait]] = t_end + rr * self.unit
        # the pops, then the pushes (slots free at the start: never a popped one)
        pop = acked | gone
        self.valid[S[pop], head[pop]] = False
        self.tries[S[pop]] = 0
        self.ready[S[pop]] = t_end
        self.c["acked"][S[acked]] += np.uint64(1)
        wp, slot, enq, bb, oo, hh = pushed
        self.valid[wp, slot] = True
        self.enq[wp, slot], self.birth[wp, slot], self.origin[wp, slot], self.hops[wp, slot] = enq, bb, oo, hh
        self.t["in_flight"] += len(wp) - int(pop.sum())

    def queues(self):
        """(origin, hops, birth, enq) [n][Q] in queue order with the unused entries zeroed, and the lengths"""
        order = np.lexsort((self.hops, self.origin, self.birth, np.where(self.valid, self.enq, BIG)), axis=-1)
        rows = np.arange(self.n)[:, None]
        v = self.valid[rows, order]
        return tuple(np.where(v, a[rows, order], 0) for a in (self.origin, self.hops, self.birth, self.enq)), self.valid.sum(axis=1)


def same(eng, host, what):
    """the device's whole table, totals and queues against the host's"""
    rows, tot = eng.fwd_read()
    for f in COUNTERS:
        assert (rows[f] == host.c[f]).all(), (what, f)
    assert (rows["ready_us"] == host.ready).all() and (rows["next"] == host.next).all() and (rows["tries"] == host.tries).all(), what
    (o, h, b, e), length = host.queues()
    assert (rows["queue_len"] == length).all() and (rows["queue_max"] == host.queue_max).all(), what
    assert tot == host.t, (what, tot, host.t)
    pk, ln = eng.fwd_queue_read()
    assert (ln == length).all() and (pk["origin"] == o).all() and (pk["hops"] == h).all() and (pk["birth_us"] == b).all() and (pk["enq_us"] == e).all(), what


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
    n, cap, check, warm = 100_000, 16384, 6, 2
    tick, air, start_at = W.TICK_US, 640, 100
    params = dict(queue_slots=8, max_retries=3, min_be=3, max_be=5, max_hops=64, backoff_unit_us=tick, seed=19)
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
    d_hop, d_par, d_root = DeviceArray(nbytes=4 * n), DeviceArray(nbytes=4 * n), DeviceArray(np.zeros(1, dtype=np.int32))
    d_src, d_cnt, d_list = DeviceArray(nbytes=4 * cap), DeviceArray(nbytes=4), DeviceArray(nbytes=4 * cap)
    inject = np.arange(5, n, 10, dtype=np.int32)
    d_inj = DeviceArray(inject)
    keep = [d_hop, d_par, d_root, d_src, d_cnt, d_list, d_inj]
    out = {"unit": "us per step; kernels: summed dispatch intervals of the k_fwd_* kernels per step", "nodes": n, "cap": cap, "air_us": air,
           "tick_us": tick, "params": params, "injected": int(len(inject))}
    try:
        totals = dev.hops_device(rsa.NB_HEARD_BY, d_root.ptr.value, 1, d_hop.ptr.value, d_par.ptr.value)
        parent = DeviceArray.read(d_par.ptr.value, np.int32, n)
        out["tree"] = dict(totals)
        dev.fwd_enable(**params)
        dev.fwd_set_next_device(d_par.ptr.value, d_root.ptr.value, 1, 0)
        dev.fwd_inject_device(d_inj.ptr.value, len(inject), 0)
        host = HostQueues(n, **params)
        host.set_next(parent, [0])
        host.inject(inject, 0)
        same(dev, host, "after the injection")
        clock = [0]

        def device_step():
            t = clock[0]
            dev.fwd_sources_device(t + start_at, cap, d_src.ptr.value, d_cnt.ptr.value)
            dev.tick_run_sources_device(t, t + tick, d_src.ptr.value, cap, t + start_at, air)
            dev.fwd_advance_device(0, None, 0)
            dev.sync()

        def host_step():
            t = clock[0]
            lst, _ = host.sources(t + start_at, cap)
            assert d_list._hip.hipMemcpy(d_list.ptr, C.c_void_p(lst.ctypes.data), C.c_size_t(lst.nbytes), 1) == 0   # H2D
            yard.tick_run_sources_device(t, t + tick, d_list.ptr.value, cap, t + start_at, air)
            want = np.where(lst >= 0, host.next[np.maximum(lst, 0)], -1).astype(np.int32)
            status = yard.unicast_query([want], fields=("status",))["status"]
            host.advance(lst, status == rsa._lib.UC_DELIVERED, t + start_at, air)

        # 1. the two routes agree, step by step, before anything is timed
        for k in range(check):
            device_step()
            host_step()
            clock[0] += tick
            same(dev, host, "check step %d" % k)
        out["checked_steps"] = check
        out["state_after_check"] = {k: int(v) for k, v in host.t.items()}
        # 2. consecutive steps, both routes in lock step (so that the yardstick's state stays the device's)
        t_dev, t_host, sendable = [], [], []
        for k in range(reps + warm):
            sendable.append(int(host.sources(clock[0] + start_at, cap)[1]))
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
        out["sendable_per_step"] = {"min": min(sendable[warm:]), "max": max(sendable[warm:])}
        # 3. the kernels' own dispatch intervals, in steps of their own
        per, launches = {}, {}
        for k in range(reps):
            dev.profile_enable(1)
            device_step()
            host_step()
            clock[0] += tick
            for name, v in dev.profile_kernels().items():
                if name.startswith("k_fwd_"):
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
