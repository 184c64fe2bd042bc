"""Reference of the measured-route query, written from the rule's text alone, and the scenes its tests
share.  Plain Python integers: entry costs, a heap Dijkstra, the parent rule (tree); a synchronous pull that counts how often a
node is lowered (pull); and the same rule in numpy for tables too large for the plain form (tree_np; tests/test_etx_ref.py holds
it to tree on every other scene).  No product code is used here."""
import heapq

import numpy as np

UNREACHED = 2 ** 64 - 1
INBOUND, BOTH = 0, 1
MODES = (INBOUND, BOTH)
FIELDS = ("cost", "parent", "slot", "link_cost", "children")
DEFAULTS = dict(mode=INBOUND, min_heard=4, max_link_cost=2048, hysteresis=192)


STATS_DTYPE = np.dtype([("heard", "<u8"), ("delivered", "<u8"), ("rssi_q8_sum", "<i8"), ("sinr_q8_sum", "<i8"), ("first_start_us", "<i8"),
                        ("last_start_us", "<i8")])


def stats(heard, delivered):
    """rm_link_stats records with these counters and everything else as a cleared entry has it"""
    s = np.zeros(heard.shape, dtype=STATS_DTYPE)
    s["heard"], s["delivered"] = heard, delivered
    s["first_start_us"], s["last_start_us"] = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    return s


def prm(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


# ---- the rule ---------------------------------------------------------------------------------------------------------------

def c_in(H, D, min_heard, cap):
    """the inbound cost of an entry, or None when it is not usable or above the cap"""
    H, D = int(H), int(D)
    if not (max(min_heard, 1) <= H <= 2 ** 40 and D >= 1):
        return None
    c = max(128, (128 * H + (D >> 1)) // D)
    return c if c <= cap else None


def combine(a, b):
    return (a * b + 64) >> 7


def link_costs(peer, heard, delivered, p):
    """c(j, k) as a list of rows, 0 where the link does not count"""
    n, K = peer.shape
    pe, H, D = peer.tolist(), heard.tolist(), delivered.tolist()
    out = [[0] * K for _ in range(n)]
    for j in range(n):
        for k in range(K):
            q = pe[j][k]
            if not (0 <= q < n) or q == j:
                continue
            c = c_in(H[j][k], D[j][k], p["min_heard"], p["max_link_cost"])
            if c is None:
                continue
            if p["mode"] == BOTH:
                back = [s for s in range(K) if pe[q][s] == j]
                if not back:
                    continue
                r = c_in(H[q][back[0]], D[q][back[0]], p["min_heard"], p["max_link_cost"])
                if r is None:
                    continue
                c = combine(c, r)
                if c > p["max_link_cost"]:
                    continue
            out[j][k] = c
    return out


def _finish(n, K, pe, lc, cost, roots, cur, hysteresis):
    """the parent rule and the totals over final costs (plain lists)"""
    parent, slot, link_cost, children = [-1] * n, [-1] * n, [0] * n, [0] * n
    kept = switched = lost = 0
    for j in range(n):
        q = cur[j] if cur is not None else -1
        valid = 0 <= q < n
        if cost[j] == UNREACHED:
            lost += valid
            continue
        if cost[j] == 0:
            continue
        pick = None
        if valid:
            held = [(lc[j][k], k) for k in range(K) if lc[j][k] and pe[j][k] == q]
            held = [(c, k) for c, k in held if cost[q] < cost[j] and cost[q] + c <= cost[j] + hysteresis]
            if held:
                c, k = min(held)
                pick = (c, q, k)
        if pick is None:
            pick = min((lc[j][k], pe[j][k], k) for k in range(K) if lc[j][k] and cost[pe[j][k]] != UNREACHED and cost[pe[j][k]] + lc[j][k] == cost[j])
        link_cost[j], parent[j], slot[j] = pick
        children[parent[j]] += 1
        if valid:
            kept += parent[j] == q
            switched += parent[j] != q
    reached = [c for c in cost if c != UNREACHED]
    totals = {"reached": len(reached), "roots": sum(c == 0 for c in reached), "kept": kept, "switched": switched, "lost": lost,
              "max_cost": max(reached) if reached else 0}
    return {"cost": np.array(cost, dtype=np.uint64), "parent": np.array(parent, dtype=np.int32), "slot": np.array(slot, dtype=np.int32),
            "link_cost": np.array(link_cost, dtype=np.uint32), "children": np.array(children, dtype=np.int32), "totals": totals}


def tree(peer, heard, delivered, p, roots, cur=None):
    """the answer by a heap Dijkstra; roots outside the table are ignored (the device form's convention)"""
    n, K = peer.shape
    pe = peer.tolist()
    lc = link_costs(peer, heard, delivered, p)
    into = [[] for _ in range(n)]   # far end -> (node, cost)
    for j in range(n):
        for k in range(K):
            if lc[j][k]:
                into[pe[j][k]].append((j, lc[j][k]))
    cost = [UNREACHED] * n
    heap = []
    for r in (int(r) for r in roots):
        if 0 <= r < n and cost[r] != 0:
            cost[r] = 0
            heap.append((0, r))
    heapq.heapify(heap)
    while heap:
        c, q = heapq.heappop(heap)
        if c != cost[q]:
            continue
        for j, w in into[q]:
            if c + w < cost[j]:
                cost[j] = c + w
                heapq.heappush(heap, (c + w, j))
    return _finish(n, K, pe, lc, cost, roots, None if cur is None else [int(v) for v in cur], p["hysteresis"])


def pull(peer, heard, delivered, p, roots):
    """synchronous pulling: every round each node takes the least cost its counting links offer over the round before's costs ->
    (cost uint64[n], rounds until nothing changes -- the last, changeless one included --, how often each node was lowered)"""
    n, K = peer.shape
    lc = np.array(link_costs(peer, heard, delivered, p), dtype=np.int64).reshape(n, K)
    big = np.int64(1) << 62
    far = np.where(lc > 0, peer, 0).astype(np.int64)
    cost = np.full(n, big, dtype=np.int64)
    valid = [int(r) for r in roots if 0 <= int(r) < n]
    cost[valid] = 0
    lowered = np.zeros(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        via = np.where((lc > 0) & (cost[far] < big), cost[far] + lc, big)
        new = np.minimum(cost, via.min(axis=1)) if K else cost
        change = new < cost
        if not change.any():
            break
        lowered += change
        cost = new
    return np.where(cost >= big, np.uint64(UNREACHED), cost.astype(np.uint64)), rounds, lowered


# ---- the same in numpy, for the wide scene ------------------------------------------------------------------------------------

def _c_in_np(H, D, p):
    H, D = H.astype(np.uint64), D.astype(np.uint64)
    usable = (H >= np.uint64(max(p["min_heard"], 1))) & (H <= np.uint64(2 ** 40)) & (D >= np.uint64(1))
    Hs, Ds = np.where(usable, H, np.uint64(1)), np.where(usable, D, np.uint64(1))
    q = np.maximum((np.uint64(128) * Hs + (Ds >> np.uint64(1))) // Ds, np.uint64(128))
    return np.where(usable & (q <= np.uint64(p["max_link_cost"])), q, np.uint64(0)).astype(np.int64)


def link_costs_np(peer, heard, delivered, p):
    n, K = peer.shape
    j = np.arange(n, dtype=np.int64)[:, None]
    pe = peer.astype(np.int64)
    ok = (pe >= 0) & (pe < n) & (pe != j)
    cin = np.where(ok, _c_in_np(heard, delivered, p), 0)
    if p["mode"] == INBOUND:
        return cin
    far = np.where(ok, pe, 0)
    match = pe[far] == j[:, :, None]              # [n][K][K]: slot s of row p holds j
    has = match.any(axis=2)
    first = match.argmax(axis=2)
    raw = _c_in_np(heard, delivered, p)
    rev = np.where(has & ok, raw[far, first], 0)
    rev = np.where((pe[far, first] == j) & ok, rev, 0)
    both = (cin * rev + 64) >> 7
    return np.where((cin > 0) & (rev > 0) & (both <= p["max_link_cost"]), both, 0)


def tree_np(peer, heard, delivered, p, roots, cur=None):
    n, K = peer.shape
    lc = link_costs_np(peer, heard, delivered, p)
    big = np.int64(1) << 62
    far = np.where(lc > 0, peer, 0).astype(np.int64)
    cost = np.full(n, big, dtype=np.int64)
    r = np.asarray(roots, dtype=np.int64).reshape(-1)
    cost[r[(r >= 0) & (r < n)]] = 0
    while True:
        via = np.where((lc > 0) & (cost[far] < big), cost[far] + lc, big)
        new = np.minimum(cost, via.min(axis=1))
        if (new == cost).all():
            break
        cost = new
    reached = cost < big
    inner = reached & (cost > 0)
    ks = np.arange(K, dtype=np.int64)[None, :]
    none = np.int64(1) << 62
    # the best rule: the least (c, p, k) as one key
    on_path = (lc > 0) & (cost[far] < big) & (cost[far] + lc == cost[:, None])
    key = np.where(on_path, (lc << 36) | (far << 4) | ks, none)
    best = key.min(axis=1)
    slot = np.where(inner, best & 15, -1)
    if cur is not None:
        q = np.asarray(cur, dtype=np.int64).reshape(-1)
        valid = (q >= 0) & (q < n)
        qs = np.where(valid, q, 0)
        ok = (lc > 0) & (far == qs[:, None]) & valid[:, None] & (cost[qs] < cost)[:, None] & (cost[qs][:, None] + lc <= (cost + p["hysteresis"])[:, None])
        kk = np.where(ok, (lc << 4) | ks, none).min(axis=1)
        keep = inner & (kk < none)
        slot = np.where(keep, kk & 15, slot)
    rows = np.arange(n)
    s = np.maximum(slot, 0)
    parent = np.where(inner, far[rows, s], -1)
    link_cost = np.where(inner, lc[rows, s], 0)
    children = np.bincount(parent[inner], minlength=n)
    kept = switched = lost = 0
    if cur is not None:
        kept = int((inner & valid & (parent == q)).sum())
        switched = int((inner & valid & (parent != q)).sum())
        lost = int((~reached & valid).sum())
    totals = {"reached": int(reached.sum()), "roots": int((cost == 0).sum()), "kept": kept, "switched": switched, "lost": lost,
              "max_cost": int(cost[reached].max()) if reached.any() else 0}
    return {"cost": np.where(reached, cost, -1).astype(np.uint64), "parent": parent.astype(np.int32), "slot": slot.astype(np.int32),
            "link_cost": link_cost.astype(np.uint32), "children": children.astype(np.int32), "totals": totals}


def same(got, tot, want, what):
    """exact equality of whatever outputs `got` holds, and of the totals"""
    for f in got:
        np.testing.assert_array_equal(got[f], want[f], err_msg="%s: %s" % (what, f))
    if tot is not None:
        assert tot == want["totals"], (what, tot, want["totals"])


# ---- scenes -------------------------------------------------------------------------------------------------------------------

def _offsets(K):
    if K == 1:
        return [-1]
    return [s * d for d in range(1, K // 2 + 1) for s in (-1, 1)]


def _rows(n, offsets, seed):
    """row j holds j + off for every offset inside the table, compacted and padded with -1; heard 40, delivered
    max(0, min(40, 40 - a * |off|)) with a drawn per entry from (0, 0, 2, 5, 9); an empty slot has cleared counters"""
    rng = np.random.default_rng(seed)
    off = np.array(offsets, dtype=np.int64)[None, :]
    far = np.arange(n, dtype=np.int64)[:, None] + off
    ok = (far >= 0) & (far < n)
    a = rng.choice(np.array([0, 0, 2, 5, 9], dtype=np.int64), size=far.shape)
    dlv = np.clip(40 - a * np.abs(off), 0, 40)
    order = np.argsort(~ok, axis=1, kind="stable")
    take = lambda x: np.take_along_axis(x, order, axis=1)
    ok = take(ok)
    peer = np.where(ok, take(far), -1).astype(np.int32)
    heard = np.where(ok, 40, 0).astype(np.uint64)
    delivered = np.where(ok, take(dlv), 0).astype(np.uint64)
    return peer, heard, delivered


def band(n, K, seed=21):
    return _rows(n, _offsets(K), seed)


def wide(seed=5):
    """131 143 nodes, K = 8: j +- 1, +- 2, +- 64, +- 4096 -- a shallow tree over many workgroups"""
    return _rows(131143, [-1, 1, -2, 2, -64, 64, -4096, 4096], seed)


BAND_P = dict(min_heard=4, max_link_cost=2000)
BANDS = ((300, 4), (3000, 8), (1025, 2), (257, 1))
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)


def _table(n, K, rows):
    """rows: {node: [(peer, heard, delivered), ...]} -> the three arrays, every other slot empty with cleared counters"""
    peer = np.full((n, K), -1, dtype=np.int32)
    heard = np.zeros((n, K), dtype=np.uint64)
    delivered = np.zeros((n, K), dtype=np.uint64)
    for j, row in rows.items():
        for k, (q, H, D) in enumerate(row):
            peer[j, k], heard[j, k], delivered[j, k] = q, H, D
    return peer, heard, delivered


def _c(c):
    """counters whose inbound cost is exactly c (c >= 128)"""
    return (c, 128)


def keep_edge():
    """hysteresis 192.  Node 3: the current parent's path exactly at cost + hysteresis (kept); 5: one unit above (switched); 6:
    the current parent at cost[q] == cost[j] (never kept, though the second condition holds); 7: the current parent in three
    slots of cost 400 (fails), 200 and 200 (the lower slot of the two); 8 and 9: cur outside the table; 0: cur at a root; 10: an
    unreached node with a valid cur (lost); 11: unreached without one; 2: cur is the best parent anyway (kept)."""
    G = (40, 40)
    rows = {1: [(0,) + G], 4: [(0,) + G], 2: [(0,) + G],
            3: [(1,) + G, (4,) + _c(320)],
            5: [(1,) + G, (4,) + _c(321)],
            6: [(1,) + G, (3,) + G],
            7: [(4,) + _c(400), (1,) + G, (4,) + _c(200), (4,) + _c(200)],
            8: [(1,) + G], 9: [(4,) + G, (1,) + G]}
    cur = np.array([1, -1, 0, 4, -1, 4, 3, 4, 99, -1, 1, -5], dtype=np.int32)
    return dict(tables=_table(12, 4, rows), roots=[0], cur=cur, prm=prm(hysteresis=192))


def cost_edge():
    """cap 2000, min_heard 4, K = 2.  Toward root 0: 1: H = D = 2^40; 2: H = 2^40 + 1; 3: H = min_heard; 4: one less; 5: D = 0; 6:
    D > H; 7: c_in exactly at the cap; 8: one above.  Pairs (near end a root): (9, 10) the product exactly at the cap while both
    halves pass; (11, 12) the product above it; (13, 14) no reverse entry; (15, 16) the reverse entry twice, the lower slot
    fails; (17, 18) twice, the lower slot counts and the upper one would not."""
    rows = {1: [(0, 2 ** 40, 2 ** 40)], 2: [(0, 2 ** 40 + 1, 2 ** 40)], 3: [(0, 4, 4)], 4: [(0, 3, 3)], 5: [(0, 40, 0)], 6: [(0, 10, 20)],
            7: [(0,) + _c(2000)], 8: [(0,) + _c(2001)],
            9: [(10,) + _c(500)], 10: [(9,) + _c(512)],
            11: [(12,) + _c(501)], 12: [(11,) + _c(512)],
            14: [(13, 40, 40)],
            15: [(16,) + _c(2001), (16, 40, 40)], 16: [(15, 40, 40)],
            17: [(18,) + _c(256), (18,) + _c(2001)], 18: [(17, 40, 40)]}
    return dict(tables=_table(19, 2, rows), roots=[0, 9, 11, 13, 15, 17], cur=None, prm=prm(max_link_cost=2000, min_heard=4))


def cost_edge_min0():
    """min_heard 0: H = 0 is still not usable (with D = 0 and with D > 0); H = 1 is"""
    rows = {1: [(0, 0, 0)], 2: [(0, 0, 5)], 3: [(0, 1, 1)]}
    return dict(tables=_table(4, 1, rows), roots=[0], cur=None, prm=prm(min_heard=0))


def junk():
    """peers -1, -7, n, 2^31 - 1 and the node itself, all with counters that would count; a far end in several slots"""
    n = 8
    G = (40, 40)
    rows = {1: [(-1,) + G, (-7,) + G, (n,) + G, (2 ** 31 - 1,) + G],
            2: [(2,) + G, (0, 40, 20), (0,) + G, (0, 40, 30)],
            3: [(3,) + G, (-2 ** 31,) + G, (2, 40, 32), (2, 40, 32)],
            4: [(n + 1,) + G, (4,) + G, (3,) + G, (2,) + _c(289)],
            0: [(2,) + G, (2, 40, 10), (0,) + G, (-1,) + G],
            5: [(6,) + G], 6: [(5,) + G]}
    cur = np.array([2, 0, 3, 2, 2, 6, 5, 7], dtype=np.int32)
    return dict(tables=_table(n, 4, rows), roots=[0], cur=cur, prm=prm(hysteresis=64))


CRAFTED = {"keep_edge": keep_edge, "cost_edge": cost_edge, "cost_edge_min0": cost_edge_min0, "junk": junk}


def root_lists(n, seed=3):
    """the root lists of the `roots` scene over a table of n nodes; "outside" is for the device form only"""
    rng = np.random.default_rng(seed)
    few = rng.choice(n, 20, replace=False)
    out = {"duplicates": [0, 0, n // 2, n // 2, 0], "none": [], "all": list(range(n))}
    for m in (16384, 16385, 40000):
        out["list%d" % m] = few[rng.integers(0, 20, m)].tolist()
    out["outside"] = [7, -1, 8, n, -2 ** 31, n - 1, 2 ** 31 - 1, 7]
    return out


def cases():
    """every scene but `wide` as (name, dict(tables, roots, cur, prm)); the bands with cur = the tree of a second draw"""
    out = []
    for n, K in BANDS:
        t = band(n, K)
        if (n, K) not in BANDS[:2]:
            out.append(("band%dx%d" % (n, K), dict(tables=t, roots=[0], cur=None, prm=prm(**BAND_P))))
            continue
        cur = tree(*band(n, K, seed=22), prm(**BAND_P), [0])["parent"]
        for h in (0, 64, 192, 1000):
            out.append(("band%dx%d_h%d" % (n, K, h), dict(tables=t, roots=[0], cur=cur, prm=prm(hysteresis=h, **BAND_P))))
    for name, make in CRAFTED.items():
        out.append((name, make()))
    t = band(300, 4)
    for label, roots in root_lists(300).items():
        if label != "outside":
            out.append(("roots_" + label, dict(tables=t, roots=roots, cur=None, prm=prm(**BAND_P))))
    for n in SIZES:
        out.append(("size%d" % n, dict(tables=band(n, 4, seed=30 + n), roots=[0], cur=None, prm=prm(**BAND_P))))
    return out
