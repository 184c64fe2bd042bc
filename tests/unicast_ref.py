"""Reference of the unicast outcome query: outcome() is the spec's table written with numpy over one
tick's result as the oracle gives it (pkt_offset, dst, verdict, rssi, sinr) and the sources the scene named.  No engine code is
involved.  Also pick_want(), the rule the tests make their wanted lists with, and the scenes' reference results, so that the CPU
tier can hold the REFERENCE ALONE to the conditions that keep the GPU tests from passing vacuously (tests/test_unicast_ref.py)."""
import numpy as np

from oracle import oracle as O

NONE, NOT_SENT, UNHEARD, INTERFERED, DELIVERED, LOST = 0, 1, 2, 3, 4, 5
NAMES = ("NONE", "NOT_SENT", "UNHEARD", "INTERFERED", "DELIVERED", "LOST")
FIELDS = ("status", "link", "rssi", "sinr", "reply_src")


def offsets(pkt, n_packets):
    """pkt_offset of packet-major links"""
    return np.searchsorted(np.asarray(pkt), np.arange(n_packets + 1)).astype(np.uint32)


def empty(n):
    return {"status": np.zeros(n, dtype=np.uint8), "link": np.full(n, -1, dtype=np.int32), "rssi": np.full(n, np.nan),
            "sinr": np.full(n, np.nan), "reply_src": np.full(n, -1, dtype=np.int32)}


def outcome(n_nodes, src, pkt_offset, dst, verdict, rssi, sinr, want, lost=False):
    """one result slot: packet p (source src[p], links [pkt_offset[p], pkt_offset[p+1])) at its wanted node want[p]; entries
    behind the slot's packets (len(want) > len(src)) are NONE.  sinr None: a medium without the column.  lost: the slot
    overflowed its link capacity."""
    want = np.asarray(want, dtype=np.int64).reshape(-1)
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    out = empty(len(want))
    for p, w in enumerate(want):
        if w < 0 or p >= len(src):
            continue
        if lost:
            out["status"][p] = LOST
            continue
        if src[p] < 0 or src[p] >= n_nodes:
            out["status"][p] = NOT_SENT
            continue
        lo, hi = int(pkt_offset[p]), int(pkt_offset[p + 1])
        hit = np.flatnonzero(np.asarray(dst[lo:hi]) == w)
        if len(hit) == 0:
            out["status"][p] = UNHEARD
            continue
        assert len(hit) == 1   # (the receivers of a frame are distinct)
        i = lo + int(hit[0])
        delivered = verdict[i] == O.DELIVERED
        out["status"][p] = DELIVERED if delivered else INTERFERED
        out["link"][p] = i
        out["rssi"][p] = rssi[i]
        if sinr is not None:
            out["sinr"][p] = sinr[i]
        if delivered:
            out["reply_src"][p] = w
    return out


def pick_want(n_nodes, src, pkt_offset, dst, verdict, first=0, host=False):
    """the tests' wanted list of one slot whose packet 0 has the flat index `first`; the class of flat index o is o % 6:
    0 first dst of the segment (node 0 if empty); 1 last dst (node n-1 if empty); 2 the o-th (mod count) DELIVERED receiver, else
    the first dst; 3 the o-th (mod count) receiver not delivered, else the middle dst; 4 the (7919 o mod count)-th node that is
    neither in the segment nor the source (n_nodes if there is none); 5 cycling through -1, the source, n_nodes, n_nodes + 5.
    host: a value >= n_nodes becomes -1 (a host list refuses it)."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    want = np.zeros(len(src), dtype=np.int32)
    for p in range(len(src)):
        o = first + p
        lo, hi = int(pkt_offset[p]), int(pkt_offset[p + 1])
        seg, ver = np.asarray(dst[lo:hi], dtype=np.int64), np.asarray(verdict[lo:hi])
        first_dst = int(seg[0]) if len(seg) else 0
        c = o % 6
        if c == 0:
            w = first_dst
        elif c == 1:
            w = int(seg[-1]) if len(seg) else n_nodes - 1
        elif c == 2:
            d = seg[ver == O.DELIVERED]
            w = int(d[o % len(d)]) if len(d) else first_dst
        elif c == 3:
            d = seg[ver != O.DELIVERED]
            w = int(d[o % len(d)]) if len(d) else (int(seg[len(seg) // 2]) if len(seg) else 0)
        elif c == 4:
            free = np.ones(n_nodes, dtype=bool)
            free[seg] = False
            if 0 <= src[p] < n_nodes:
                free[src[p]] = False
            f = np.flatnonzero(free)
            w = int(f[(7919 * o) % len(f)]) if len(f) else n_nodes
        else:
            w = (-1, int(src[p]), n_nodes, n_nodes + 5)[(o // 6) % 4]
        want[p] = -1 if (host and w >= n_nodes) else w
    return want


class Slot:
    """one tick's reference result in the shape outcome() and pick_want() take"""

    def __init__(self, n_nodes, src, res, verdict=None):
        self.n_nodes = n_nodes
        self.src = np.asarray(src, dtype=np.int32).reshape(-1)
        self.count = int(res.count)
        self.dst, self.rssi = np.asarray(res.dst), np.asarray(res.rssi)
        self.verdict = np.asarray(res.verdict if verdict is None else verdict)
        self.sinr = None if res.sinr is None else np.asarray(res.sinr)
        self.pkt_offset = offsets(res.pkt, len(self.src))

    def want(self, first=0, host=False):
        return pick_want(self.n_nodes, self.src, self.pkt_offset, self.dst, self.verdict, first, host)

    def outcome(self, want, lost=False, sinr=True):
        return outcome(self.n_nodes, self.src, self.pkt_offset, self.dst, self.verdict, self.rssi, self.sinr if sinr else None, want, lost)


def flat(outs):
    """the outcomes of several slots, flat in slot order (link stays a position in its own slot)"""
    return {f: np.concatenate([o[f] for o in outs]) if outs else empty(0)[f] for f in FIELDS}


def wants(slots, host=False):
    """the pick rule over the slots of a call, flat packet index running through them"""
    out, first = [], 0
    for s in slots:
        out.append(s.want(first, host))
        first += len(s.src)
    return out


def counts(status):
    return np.bincount(np.asarray(status), minlength=6)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def equal(got, want, what="", fields=FIELDS, link=True):
    """exact: status, link, rssi bits, sinr bits, reply_src"""
    for f in fields:
        if f == "link" and not link:
            continue
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if f in ("rssi", "sinr"):
            g, w = bits(g), bits(w)
        np.testing.assert_array_equal(g, w, err_msg="%s: %s" % (what, f))


# ---- the scenes' reference results ---------------------------------------------------------------------------------------------

def sinr_slots(nd, lists, starts, air, em_seed=None, t_begin=None):
    """errmodel_ref.Replay over ticks of source lists on the SINR medium -> [Slot] (em_seed None: the verdicts before E10)"""
    import errmodel_ref as R
    rep = R.Replay(nd, seed=R.SEED if em_seed is None else em_seed)
    out = []
    for k, (l, s) in enumerate(zip(lists, starts)):
        w, _ = rep.tick(s if t_begin is None else t_begin[k], l, s, air[k] if isinstance(air, (list, tuple)) else air)
        out.append(Slot(nd.n, l, w, verdict=w.plain if em_seed is None else None))
    return out


def media_slot(scene):
    """a stats_ref scene of one of the reference's media -> Slot (sinr: no column)"""
    import stats_ref as S
    nd, _, _, pk, _, _ = scene
    res = S.oracle_tick(scene)
    s = Slot(nd.n, pk["src"], res)
    s.sinr = None
    s.res = res
    return s


def ack_round_trip(nd, srcs, em_seed=None):
    """the acknowledgement round trip of DESIGN.md E12 on errmodel_ref.scene_lone: the data tick at 0 with air 4064, want chosen
    greedily in packet order (a DELIVERED receiver not chosen yet; every fourth packet an unheard node instead), the reply list as
    the acknowledgement tick's source list at 4256 with air 352, queried with want[k] = data source k
    -> (data Slot, want, data outcome, ack Slot, ack want, ack outcome)"""
    import errmodel_ref as R
    rep = R.Replay(nd, seed=R.SEED if em_seed is None else em_seed)
    w, _ = rep.tick(0, srcs, 0, 4064)
    data = Slot(nd.n, srcs, w, verdict=w.plain if em_seed is None else None)
    want, taken = np.full(len(srcs), -1, dtype=np.int32), set()
    for p in range(len(srcs)):
        lo, hi = int(data.pkt_offset[p]), int(data.pkt_offset[p + 1])
        seg = data.dst[lo:hi]
        if p % 4 == 3:
            free = np.ones(nd.n, dtype=bool)
            free[seg] = False
            free[srcs[p]] = False
            want[p] = int(np.flatnonzero(free)[(7919 * p) % int(free.sum())])
            continue
        for i in range(lo, hi):
            if data.verdict[i] == O.DELIVERED and int(data.dst[i]) not in taken:
                want[p] = int(data.dst[i])
                taken.add(want[p])
                break
    d_out = data.outcome(want)
    reply = d_out["reply_src"]
    a, _ = rep.tick(4256, reply, 4256, 352)
    ack = Slot(nd.n, reply, a, verdict=a.plain if em_seed is None else None)
    a_want = np.asarray(srcs, dtype=np.int32)
    return data, want, d_out, ack, a_want, ack.outcome(a_want)
