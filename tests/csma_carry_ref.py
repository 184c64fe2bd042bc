"""Expected values of the carry of a CSMA-CA gated batch: a Python restatement of the schedule with carried
packets, of the carry-out (collect) and of the rule that merges the parts of a split batch into one outcome per packet; and what the
oracle's run over the WHOLE tick range (tests/csma_ref.py::Run) says a cut carries.  No engine code is involved.

The whole and the split differ in one thing, which `live` restates: E8 schedules every attempt of every packet, made or not, so the whole
run keeps a padding slot for each later attempt of a packet that was sent already.  A carry holds pending packets only: in the part
after a cut those DEAD slots of packets from before the cut do not exist.  Nothing is sensed or sent in a dead slot; packet numbers of
the split are positions among the surviving slots, in the same order, and everything else is the whole's."""
import numpy as np

import csma_ref as SR

CARRY = np.dtype([("origin_cca_time_us", "<i8"), ("origin_slot", "<i4"), ("node", "<i4"), ("tick", "<i4"), ("attempt", "<i4")])


def carry_list(rows):
    """[(origin_cca_time_us, origin_slot, node, tick, attempt)] -> a CARRY array"""
    a = np.zeros(len(rows), dtype=CARRY)
    for i, row in enumerate(rows):
        a[i] = tuple(int(v) for v in row)
    return a


def schedule(p, n_src, t_cca, carry):
    """-> per tick the expanded list as [(packet, attempt, tick of the next attempt or -1)]: own entries, then the carried packets'
    attempts in carry-list order, then the own packets' retries by (origin tick, origin slot).  Packet: the flat index over the own
    lists, or sum(n_src) + c for carried packet c."""
    n_ticks = len(n_src)
    n_pkt = int(np.sum(n_src))
    base = SR.schedule(p, n_src, t_cca)
    carried = [[] for _ in range(n_ticks)]
    for c, r in enumerate(carry):
        tick, k, t0 = int(r["tick"]), int(r["origin_slot"]), int(r["origin_cca_time_us"])
        if tick >= n_ticks:
            continue
        for a in range(int(r["attempt"]), p.max_backoffs + 1):
            nxt = tick + 1 + SR.backoff(p, t0, k, a) if a < p.max_backoffs else -1
            carried[tick].append((n_pkt + c, a, nxt))
            if nxt < 0 or nxt >= n_ticks:
                break
            tick = nxt
    out = []
    for b in range(n_ticks):
        assert carried[b] == sorted(carried[b])                # a packet has one attempt per tick: list order is the order of the index
        own = int(n_src[b])
        out.append(base[b][:own] + carried[b] + base[b][own:])
    return out


def collect(lists, t_cca, carry, out, carried_out):
    """the carry-out: the PENDING carried packets in carry-in order, then the PENDING own packets in flat order, each with
    tick - n_ticks and attempt = attempts.  -> (CARRY array, [("c", carry index) or ("o", flat own index)] per entry)"""
    n_ticks = len(lists)
    rows, who = [], []
    for c, r in enumerate(carry):
        if carried_out["status"][c] == SR.PENDING:
            rows.append((r["origin_cca_time_us"], r["origin_slot"], r["node"], int(carried_out["tick"][c]) - n_ticks, carried_out["attempts"][c]))
            who.append(("c", c))
    o = 0
    for b, src in enumerate(lists):
        for k, j in enumerate(src):
            if out["status"][o] == SR.PENDING:
                rows.append((t_cca[b], k, j, int(out["tick"][o]) - n_ticks, out["attempts"][o]))
                who.append(("o", o))
            o += 1
    return carry_list(rows), who


class Merge:
    """The parts of a split batch as one: per packet of the WHOLE (flat index over all parts' own lists) the entry of the part in which
    it stopped being pending, with ticks counted from the whole's first tick; flags and energy from the last part in which it made an
    attempt (a part in which a carried packet has no slot leaves them alone)."""

    def __init__(self, n_pkt):
        self.status = np.full(n_pkt, SR.TRYING, dtype=np.uint8)
        self.attempts = np.zeros(n_pkt, dtype=np.uint8)
        self.tick = np.full(n_pkt, -1, dtype=np.int32)
        self.pkt = np.full(n_pkt, -1, dtype=np.int32)
        self.flags = np.zeros(n_pkt, dtype=np.uint8)
        self.energy = np.full(n_pkt, np.nan)
        self.done = 0                # own packets of the parts so far
        self.ids = []                # the whole's packet of every entry of the current carry list
        self.times_carried = np.zeros(n_pkt, dtype=np.int32)

    def _take(self, g, first_tick, t, i):
        made = int(t["attempts"][i]) > int(self.attempts[g])
        self.status[g], self.attempts[g], self.pkt[g] = t["status"][i], t["attempts"][i], t["pkt"][i]
        self.tick[g] = first_tick + int(t["tick"][i]) if t["tick"][i] >= 0 else -1
        if made or self.status[g] == SR.NONE:
            self.flags[g], self.energy[g] = t["flags"][i], t["energy_dbm"][i]

    def part(self, first_tick, n_own, out, carried_out, who):
        """a part's two tables, and its carry-out as collect names it (who) -> the whole's packets of that carry-out"""
        assert len(carried_out["status"]) == len(self.ids) and len(out["status"]) == n_own
        for c, g in enumerate(self.ids):
            assert self.status[g] == SR.PENDING
            self._take(g, first_tick, carried_out, c)
        for o in range(n_own):
            self._take(self.done + o, first_tick, out, o)
        nxt = [self.ids[i] if kind == "c" else self.done + i for kind, i in who]
        self.times_carried[nxt] += 1
        self.done += n_own
        self.ids = nxt
        return nxt

    def outcome(self):
        return np.stack([self.status.astype(np.int64), self.attempts.astype(np.int64), self.tick.astype(np.int64), self.pkt.astype(np.int64),
                         self.flags.astype(np.int64)])


def live(r, first, last, carry_ids):
    """per tick first .. last-1 of the whole run: the indices of its slots that the part first .. last-1 has too (the part's own packets
    and the packets carried into it), in order -- the part's slot s of tick T is the whole's slot live[T - first][s]"""
    before = sum(len(s) for s in r.lists[:first])
    keep = set(carry_ids)
    return [np.array([i for i, (o, _, _) in enumerate(r.sched[T]) if o >= before or o in keep], dtype=np.int64) for T in range(first, last)]


def expected_links(exp, alive):
    """a tick's heard links of the whole (cca_ref.Expected) under the part's packet numbers"""
    import cca_ref as CR
    rank = {int(i): k for k, i in enumerate(alive)}
    return CR.Expected(len(alive), np.array([rank[int(i)] for i in exp.slots], dtype=np.int64), exp.raw, exp.new)


def whole_pkt(r, cuts):
    """r.pkt under the split's packet numbers: a sent packet's position among the live slots of its tick, in the part that holds the tick"""
    edges = [0] + list(cuts) + [len(r.lists)]
    out = r.pkt.copy()
    for first, last in zip(edges[:-1], edges[1:]):
        ids = _pending_at(r, first)
        alive = live(r, first, last, ids)
        for o in np.flatnonzero((r.status == SR.SENT) & (r.tick >= first) & (r.tick < last)):
            out[o] = int(np.searchsorted(alive[int(r.tick[o]) - first], r.pkt[o]))
    return out


def _pending_at(r, cut):
    found = set()
    for T in range(cut):
        for i, (o, a, nxt) in enumerate(r.sched[T]):
            if r.made[T][i] >= 0 and r.kept[T][i] < 0 and nxt >= cut:
                found.add(o)
    return sorted(found)


def tables_of(r, first, last, carry_ids, cut_carry):
    """What the oracle's whole run `r` says the part over its ticks first .. last-1 reports: (own table, carried table), each a dict of
    the six fields, ticks relative to `first`, packet numbers the part's (live).  carry_ids / cut_carry: the part's carry-in (carry_at(r, first)).  A packet's entry is
    that of its last made attempt before `last`."""
    n_pkt_before = sum(len(s) for s in r.lists[:first])
    n_own = sum(len(s) for s in r.lists[first:last])
    ids = list(carry_ids) + list(range(n_pkt_before, n_pkt_before + n_own))
    n = len(ids)
    t = {"status": np.zeros(n, dtype=np.uint8), "attempts": np.zeros(n, dtype=np.uint8), "tick": np.full(n, -1, dtype=np.int32),
         "pkt": np.full(n, -1, dtype=np.int32), "flags": np.zeros(n, dtype=np.uint8), "energy_dbm": np.full(n, np.nan)}
    at = {g: i for i, g in enumerate(ids)}
    alive = live(r, first, last, carry_ids)
    for c in range(len(carry_ids)):                            # no slot in this part: still pending, as it came in
        t["status"][c], t["attempts"][c], t["tick"][c] = SR.PENDING, cut_carry["attempt"][c], cut_carry["tick"][c]
    for T in range(first, last):
        for i, (o, a, nxt) in enumerate(r.sched[T]):
            if o not in at or r.made[T][i] < 0:
                continue
            e = at[o]
            t["attempts"][e], t["flags"][e], t["energy_dbm"][e] = a + 1, r.slot_flags[T][i], r.slot_energy[T][i]
            if r.kept[T][i] >= 0:
                t["status"][e], t["tick"][e], t["pkt"][e] = SR.SENT, T - first, int(np.searchsorted(alive[T - first], i))
            elif nxt < 0:
                t["status"][e], t["tick"][e] = SR.FAILED, -1
            elif nxt >= last:
                t["status"][e], t["tick"][e] = SR.PENDING, nxt - first
    k = len(carry_ids)
    return {f: a[k:] for f, a in t.items()}, {f: a[:k] for f, a in t.items()}


def carry_at(r, cut, t_cca):
    """What the oracle's whole run says is carried over a cut before tick `cut`: the packets of ticks < cut whose last made attempt before
    the cut was deferred with the next one at or behind it (t_cca: the ticks' sample times).  -> (CARRY array with ticks relative to `cut`, the packets' flat indices),
    in (origin tick, origin slot) order -- the order collect gives by induction."""
    first = np.concatenate([[0], np.cumsum([len(s) for s in r.lists])]).astype(np.int64)
    found = {}
    for T in range(cut):
        for i, (o, a, nxt) in enumerate(r.sched[T]):
            if r.made[T][i] >= 0 and r.kept[T][i] < 0 and nxt >= cut:
                found[o] = (nxt - cut, a + 1)
    rows, ids = [], []
    for o in sorted(found):
        b = int(np.searchsorted(first, o, side="right")) - 1
        k = o - int(first[b])
        rows.append((t_cca[b], k, r.lists[b][k], found[o][0], found[o][1]))
        ids.append(o)
    return carry_list(rows), ids
