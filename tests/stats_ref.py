"""Reference of the per-node traffic counters: the eight columns accumulated with numpy from the
oracle's per-tick results (pkt, dst, verdict, pkt_interference) and the sources and air times the scene named.  No engine code
is involved.  Also the scenes the GPU tests of the counters use beyond those of errmodel_ref / csma_ref, so that the CPU tier
can hold the REFERENCE ALONE to the conditions that make those scenes worth running (tests/test_stats_ref.py)."""
import numpy as np

from oracle import oracle as O
from util import oracle_model

COLS = ("tx_frames", "tx_failed", "tx_air_us", "tx_links_heard", "tx_links_delivered", "rx_heard", "rx_delivered", "rx_air_us")
DTYPE = np.dtype([(c, "<u8") for c in COLS])


class Table:
    """the table after a sequence of evaluated ticks, and the totals"""

    def __init__(self, n):
        self.n = n
        self.t = np.zeros(n, dtype=DTYPE)
        self.counted = self.skipped = 0

    def add(self, src, air_us, failed, pkt, dst, verdict):
        """one evaluated tick: its new frames in packet order (src outside 0 .. n-1: padding, a deferred candidate, a slot not
        made), their Tx-failure flags, and its heard links (pkt: the frame's position in that order)"""
        src = np.asarray(src, dtype=np.int64).reshape(-1)
        if len(src) == 0:
            return  # an empty tick changes nothing
        self.counted += 1
        air = np.broadcast_to(np.asarray(air_us, dtype=np.int64), src.shape).astype(np.uint64)
        failed = np.asarray(failed, dtype=np.uint64).reshape(-1)
        pkt, dst = np.asarray(pkt, dtype=np.int64), np.asarray(dst, dtype=np.int64)
        deliv = (np.asarray(verdict) == O.DELIVERED).astype(np.uint64)
        one = np.uint64(1)
        ok = (src >= 0) & (src < self.n)
        np.add.at(self.t["tx_frames"], src[ok], one)
        np.add.at(self.t["tx_air_us"], src[ok], air[ok])
        np.add.at(self.t["tx_failed"], src[ok], failed[ok])
        np.add.at(self.t["rx_heard"], dst, one)
        np.add.at(self.t["rx_air_us"], dst, air[pkt])
        np.add.at(self.t["rx_delivered"], dst, deliv)
        lk = ok[pkt]
        np.add.at(self.t["tx_links_heard"], src[pkt][lk], one)
        np.add.at(self.t["tx_links_delivered"], src[pkt][lk], deliv[lk])

    def skip(self):
        self.skipped += 1

    def add_result(self, new, res, verdict=None):
        """a tick of oracle packets `new` (padding: src -1) with a TickResult whose pkt counts the positions of `new`
        (errmodel_ref.Replay's, or the oracle's own over packets without padding); verdict: another final verdict column"""
        new = np.atleast_1d(new)
        self.add(new["src"], new["air_us"], res.pkt_interference, res.pkt, res.dst, res.verdict if verdict is None else verdict)

    def add_expected(self, exp, n_slots, verdict=None):
        """a tick as cca_ref.Expected has it (csma_ref.Run.exp, cca_batch_ref.Run.exp): exp.new are the frames of the live slots,
        exp.raw the oracle's result over them; n_slots: the slots of the tick's list (0: an empty tick)"""
        if n_slots <= 0:
            return
        if exp.raw is None:   # slots, but not one frame: a counted tick that adds nothing
            self.counted += 1
            return
        self.add(exp.new["src"], exp.new["air_us"], exp.raw.pkt_interference, exp.raw.pkt, exp.raw.dst,
                 exp.raw.verdict if verdict is None else verdict)

    def totals(self):
        return {"ticks_counted": self.counted, "ticks_skipped": self.skipped}


def equal(got, want, what=""):
    """exact integer equality of whole tables (got: the engine's structured array)"""
    assert got.dtype.names == COLS, got.dtype
    assert len(got) == len(want.t), (what, len(got), len(want.t))
    for c in COLS:
        np.testing.assert_array_equal(got[c], want.t[c], err_msg="%s: column %s" % (what, c))


# ---- what a scene has to show (tests/test_stats_ref.py) --------------------------------------------------------------------

def run_lengths(pkt):
    """heard links per frame, in the order of the packet-major arrays"""
    pkt = np.asarray(pkt)
    if len(pkt) == 0:
        return np.zeros(0, dtype=np.int64)
    cut = np.flatnonzero(np.diff(pkt)) + 1
    return np.diff(np.concatenate([[0], cut, [len(pkt)]]))


def most_packets_in_a_wave(pkt):
    """the largest number of distinct packets among 64 consecutive links at a multiple of 64 (what one wave of the pass sees)"""
    pkt = np.asarray(pkt)
    return max([len(np.unique(pkt[i:i + 64])) for i in range(0, len(pkt), 64)], default=0)


# ---- scenes of the reference's media -------------------------------------------------------------------------------------

def _uniform(n, side, seed):
    rng = np.random.default_rng(seed)
    nd = O.NodeTable(n)
    nd.x, nd.y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    return nd, rng


AIR = 4064


def scene_udgm():
    """stochastic UDGM: 2500 nodes, about six in transmission range, 300 frames, both ratios below 1:
    -> nd, kind, params, packets, matrix, seed"""
    n = 2500
    nd, rng = _uniform(n, 50.0 * np.sqrt(np.pi * n / 6.0), 31)
    src = rng.choice(n, 300, replace=False).astype(np.int32)
    return nd, "udgm", {"udgm_success_ratio_tx": 0.8, "udgm_success_ratio_rx": 0.7}, nd.packets(src, 0, AIR), None, 2024


def scene_udgm_const():
    """UDGM constant loss: 2000 nodes, 200 frames, no draws"""
    n = 2000
    nd, rng = _uniform(n, 50.0 * np.sqrt(np.pi * n / 20.0), 32)
    src = rng.choice(n, 200, replace=False).astype(np.int32)
    return nd, "udgm_const", {}, nd.packets(src, 0, AIR), None, None


def scene_n2n():
    """a node-to-node matrix with fractional node probabilities: the draws run, and the tick takes the unsorted table's path"""
    n = 300
    rng = np.random.default_rng(8)
    nd, _ = _uniform(n, 100.0, 3)
    m = np.where(rng.random((n, n)) < 0.1, rng.uniform(0, 1.3, (n, n)), 0.0)
    nd.int_id[:] = np.arange(1, n + 1)
    nd.int_id[5] = -1
    nd.int_id[6] = n + 7
    nd.rxprob[10:20] = 0.5
    nd.txprob[30:40] = 0.7
    src = rng.choice(n, 60, replace=False).astype(np.int32)
    return nd, "n2n", {}, nd.packets(src, 0, AIR), m, 11


def scene_null():
    """the Null medium (every node hears every frame): the tick takes the dense form"""
    n = 3000
    nd, rng = _uniform(n, 400.0, 33)
    src = np.sort(rng.choice(n, 6, replace=False)).astype(np.int32)
    return nd, "null", {}, nd.packets(src, 0, AIR), None, None


def oracle_tick(scene):
    nd, kind, params, pk, matrix, seed = scene
    state = O.lib().orc_jrandom_seed(seed) if seed is not None else 0
    return O.tick(oracle_model(O, kind, params, matrix), nd, pk, rng_state=state, cap=1 << 22)


def table_of(scene, res=None):
    nd, _, _, pk, _, _ = scene
    t = Table(nd.n)
    t.add_result(pk, oracle_tick(scene) if res is None else res)
    return t
