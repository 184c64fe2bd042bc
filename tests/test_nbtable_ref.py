"""The neighbour tables without a GPU: the scenes of tests/nbtable_ref.py held to the conditions that make
them worth running -- from the reference alone --, and the pure host functions rm_nbtable_from_result, rm_nbtable_expire_tables,
rm_nbtable_validate and rm_nbtable_defaults against the reference, exactly: over every scene (a driver that sends every call to
the host rule as well) and over crafted results with NaN and weak links, sources outside the table, duplicates and pins."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import linkstats_ref as LS
import nbtable_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


# ---- the reference alone: every scene shows what it is there for -------------------------------------------------------------------

def plain(O):
    return lambda *a, **kw: R.Driver(*a, **kw)


def full_rows(d):
    peer = d.ref.tab.peer
    return int(((peer >= 0).all(axis=1)).sum())


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("shape", ["line", "clique"])
def test_fill_conditions(O, shape, n, K):
    d = R.scene_fill(plain(O), shape, n, K)
    log, tot = d.ref.log, d.ref.totals()
    assert tot["updates"] == 8 and tot["admitted"] == log["empty"] >= n and tot["evicted_stale"] == tot["evicted_poor"] == 0
    assert max(d.ref.cnt["admitted"]) <= min(K, 8)            # (one admission per node and tick, never more than the row holds)
    assert log["ties"] >= n // 2
    if shape == "clique":
        assert full_rows(d) == n and (log["refused"] > 0) == (K < 8)
    else:
        assert (log["refused"] > 0) == (K < 8)                 # (three neighbours on either side)
    held = d.ref.tab.t["heard"][d.ref.tab.peer >= 0]
    assert (held >= 1).all() and (held >= 2).any()             # (step 3 counted the admitting frame; E14 the later ones)


def test_tie_goes_to_the_least_source(O):
    d = R.scene_tie(plain(O))
    assert d.ref.log["ties"] >= 1 and int(d.ref.tab.peer[0, 0]) == 1
    assert int(d.ref.tab.t["heard"][0, 0]) == 1


def test_long_conditions(O):
    d = R.scene_long(plain(O))
    assert d.ref.log["bids"] >= 18336 and d.ref.totals()["admitted"] == 2 * 192


@pytest.mark.parametrize("n", [1025, 4097])
def test_big_conditions(O, n):
    d = R.scene_big(plain(O), n)
    tot = d.ref.totals()
    assert tot["admitted"] > n // 2 and tot["expired"] > n // 8 and tot["refused"] >= 0
    assert (d.ref.tab.peer >= 0).any()                         # (not everything expired)
    assert d.ref.cnt["expired"][n - 1] + d.ref.cnt["admitted"][n - 1] + sum(d.ref.cnt["admitted"][1024:]) > 0   # (the ragged last workgroup works)


def test_media_conditions(O):
    a, b = R.scene_media(plain(O), 1), R.scene_media(plain(O), 0)
    for d in (a, b):
        assert d.ref.log["undelivered_bidders"] >= 10 and d.ref.log["low"] >= 10 and d.ref.log["ties"] >= 1
        assert ((d.ref.tab.t["delivered"] < d.ref.tab.t["heard"])).any()
    assert a.ref.log["undelivered_admitted"] == 0 and b.ref.log["undelivered_admitted"] >= 1
    assert a.ref.tab.peer.tobytes() != b.ref.tab.peer.tobytes()


def test_evict_conditions(O):
    d = R.scene_evict(plain(O))
    log = d.ref.log
    assert log["empty"] >= 1 and log["stale"] >= 1 and log["stale_choice"] >= 1
    assert d.ref.tab.peer[0].tolist() == [3, 2] and d.ref.cnt["evicted_stale"][0] == 1


def test_poor_conditions(O):
    d = R.scene_poor(plain(O))
    log = d.ref.log
    assert log["poor"] >= 1 and log["poor_zero_first"] >= 1 and log["refused_pinned"] >= 1 and log["undelivered_admitted"] >= 1


def test_pins_and_disabled_lines(O):
    d = R.scene_pins(plain(O))
    assert d.ref.log["refused_pinned"] >= 3 and d.ref.log["stale"] == 1 and int(d.ref.tab.peer[4, 0]) == 2
    assert d.ref.totals()["expired"] == 0 and d.ref.totals()["refused"] >= 7
    d = R.scene_disabled(plain(O))
    tot = d.ref.totals()
    assert tot["expired"] == 0 and tot["evicted_stale"] == tot["evicted_poor"] == 0 and tot["refused"] >= 8


def test_capacity_dup_weak(O):
    d = R.scene_capacity(plain(O))
    assert d.unchanged and d.ref.totals()["skipped_slots"] == 1 and d.ref.tab.skipped == 1
    d = R.scene_dup(plain(O))
    assert d.ref.log["dup_counted"] == 3 and (d.ref.tab.t["heard"][[0, 2, 3], 0] == 2).all()
    d = R.scene_weak(plain(O))
    assert d.ref.log["low"] >= 8 and (np.abs(d.ref.tab.peer - np.arange(8)[:, None])[d.ref.tab.peer >= 0] == 1).all()


def test_batch_against_lone_ticks(O):
    """both orders are deterministic; a peer admitted from slot b of a batch misses its frames of the later slots"""
    a, b = R.scene_batch(plain(O), True), R.scene_batch(plain(O), False)
    assert a.ref.tab.peer.tobytes() == b.ref.tab.peer.tobytes()
    assert (a.ref.tab.t["heard"] != b.ref.tab.t["heard"]).any() and (a.ref.tab.t["heard"] <= b.ref.tab.t["heard"]).all()


# ---- the host functions against the reference ---------------------------------------------------------------------------------------

def params_of(rsa, p):
    return rsa.Engine.nbtable_params(**{k: v for k, v in p.items() if k != "reserved"})


def host_result(res):
    """a Result as rm_host_result's columns"""
    return types.SimpleNamespace(count=len(res.dst), pkt_offset=np.array(res.pkt_offset, dtype=np.uint32), dst=np.array(res.dst, dtype=np.int32),
                                 verdict=np.array(res.verdict, dtype=np.uint8), rssi=np.array(res.rssi, dtype=np.float64),
                                 sinr=None if res.sinr is None else np.array(res.sinr, dtype=np.float64))


class HostDriver(R.Driver):
    """every update and expire to the host rule as well, on its own tables; compared after every call"""

    def __init__(self, rsa, *a, **kw):
        super().__init__(*a, **kw)
        self.rsa = rsa
        self.prm = params_of(rsa, self.ref.p)
        n, K = self.nd.n, self.K
        self.peer = np.full((n, K), -1, dtype=np.int32)
        self.stats = np.zeros((n, K), dtype=rsa._lib.LINK_STATS_DTYPE)
        self.stats[...] = LS.CLEARED
        self.node = np.zeros(n, dtype=rsa._lib.NBTABLE_NODE_DTYPE)
        self.tot = np.zeros(1, dtype=rsa._lib.NBTABLE_TOTALS_DTYPE)

    def tick(self, *a):
        res = super().tick(*a)
        # E14's pass is not under test here: the host tables take the reference's
        self.peer[...] = self.ref.tab.peer
        self.stats[...] = self.ref.tab.t
        return res

    def update(self, res, time_us, pin=None, slot=0):
        if res.lost:
            self.tot["skipped_slots"] += 1       # (a host result has no lost flag: the caller's)
        else:
            self.rsa.Engine.nbtable_from_result(host_result(res), res.src, res.start, self.peer, self.stats, self.prm, time_us, pin, self.node, self.tot)
        super().update(res, time_us, pin, slot)

    def expire(self, time_us, pin=None):
        self.rsa.Engine.nbtable_expire_tables(self.peer, self.stats, self.prm, time_us, pin, self.node, self.tot)
        super().expire(time_us, pin)

    def watch(self, nodes, rows):
        self.ref.tab.watch(nodes, rows)
        self.peer[...] = self.ref.tab.peer
        self.stats[...] = self.ref.tab.t
        self.after("watch")

    def after(self, what):
        super().after(what)
        same_tables(self.ref, self.peer, self.stats, self.node, self.tot, what)


def same_tables(ref, peer, stats, node, tot, what):
    np.testing.assert_array_equal(peer, ref.tab.peer, err_msg=what + ": peer")
    LS.equal(stats, ref.tab, what)
    for f in R.NODE_FIELDS:
        assert node[f].tolist() == ref.cnt[f], (what, f)
    assert {k: int(tot[k][0]) for k in tot.dtype.names} == ref.totals(), what


SCENES = [lambda m: R.scene_fill(m, "line", 65, 2), lambda m: R.scene_fill(m, "clique", 64, 4), lambda m: R.scene_fill(m, "clique", 65, 1),
          lambda m: R.scene_fill(m, "line", 64, 8), R.scene_tie, lambda m: R.scene_big(m, 1025), lambda m: R.scene_media(m, 0),
          lambda m: R.scene_media(m, 1), R.scene_evict, R.scene_poor, R.scene_pins, R.scene_disabled, R.scene_capacity, R.scene_dup, R.scene_weak,
          lambda m: R.scene_batch(m, True), lambda m: R.scene_batch(m, False)]


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_host_rule_over_the_scenes(rsa, O, k):
    d = SCENES[k](lambda *a, **kw: HostDriver(rsa, *a, **kw))
    assert d.steps >= 1


def crafted(rng, n, K):
    """a result and tables no medium gives: NaN, infinite and weak rssi, sources outside the table and equal to the receiver,
    duplicate sources, empty packets; rows with stale, poor, never-delivered, self and out-of-table entries"""
    n_pkt = int(rng.integers(1, 7))
    src = rng.integers(-2, n + 2, n_pkt)
    if n_pkt > 2:
        src[2] = src[0]
    start = rng.integers(0, 50_000, n_pkt)
    dst, off = [], [0]
    for p in range(n_pkt):
        m = int(rng.integers(0, n + 1)) if p != 1 else 0
        dst += sorted(rng.choice(np.arange(-1, n + 1), size=min(m, n + 2), replace=False).tolist())
        off.append(len(dst))
    L = len(dst)
    rssi = rng.choice([-70.0, -70.0, -80.5, -94.99, -95.0, -95.01, -120.0, np.nan, np.inf, -np.inf, 3e9, -3e9], size=L)
    sinr = rng.choice([1.5, -3.25, np.nan, 40.0], size=L)
    verdict = rng.choice([1, 2, 2], size=L)
    res = R.Result(src, start, off, dst, verdict, rssi, sinr if rng.integers(0, 2) else None)
    peer = np.zeros((n, K), dtype=np.int32)
    for d in range(n):                                          # (a row's valid entries are distinct; one slot in twelve holds junk)
        peer[d] = rng.permutation([j for j in range(n) if j != d])[:K]
        junk = rng.integers(0, 12, K) == 0
        peer[d, junk] = rng.choice([-1, -2, n, d], size=int(junk.sum()))
    t = np.zeros((n, K), dtype=LS.DTYPE)
    t["heard"] = rng.choice([0, 1, 2, 4, 9, 1 << 58], size=(n, K))
    t["delivered"] = np.minimum(t["heard"], rng.choice([0, 0, 1, 3, 9], size=(n, K)).astype(np.uint64))
    t["last_start_us"] = rng.choice([LS.I64_MIN, 0, 10_000, 10_000, 40_000, 90_000], size=(n, K))
    t["first_start_us"] = np.where(t["last_start_us"] == LS.I64_MIN, LS.I64_MAX, 0)
    pin = None if rng.integers(0, 3) == 0 else rng.integers(-3, n, n).astype(np.int32)
    return res, peer, t, pin


@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_host_rule_over_crafted_results(rsa, K):
    rng = np.random.default_rng(100 + K)
    n = 12
    seen = {k: 0 for k in ("nan", "low", "stale", "stale_choice", "poor", "poor_zero_first", "refused", "refused_pinned", "empty", "ties",
                           "undelivered_admitted", "dup_counted")}
    for trial in range(300):
        prm = dict(admit_rssi_dbm=-95.0, timeout_us=int(rng.choice([0, 30_000, 200_000])), min_heard=int(rng.choice([0, 2, 5])),
                   evict_cost=int(rng.choice([0, 128, 200, 1024])), require_delivered=int(rng.integers(0, 2)))
        res, peer, t, pin = crafted(rng, n, K)
        ref = R.State(n, K, **prm)
        ref.tab.peer[...] = peer
        ref.tab.t[...] = t
        time_us = int(rng.choice([0, 20_000, 60_000, 100_000]))
        stats = t.copy()
        node, tot = rsa.Engine.nbtable_from_result(host_result(res), res.src, res.start, peer, stats, params_of(rsa, prm), time_us, pin)
        ref.update(res, time_us, pin)
        ref.check()
        same_tables(ref, peer, stats, node, tot, "update, trial %d" % trial)
        rsa.Engine.nbtable_expire_tables(peer, stats, params_of(rsa, prm), time_us + 5_000, pin, node, tot)
        ref.expire(time_us + 5_000, pin)
        same_tables(ref, peer, stats, node, tot, "expire, trial %d" % trial)
        for k in seen:
            seen[k] += ref.log[k]
    missing = [k for k, v in seen.items() if v < 1 and not (K == 1 and k in ("stale_choice", "poor_zero_first"))]
    assert not missing, missing


def test_defaults_and_validate(rsa):
    p = rsa.Engine.nbtable_params()
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS and rsa.Engine.nbtable_validate(p) == 0
    cases = [dict(admit_rssi_dbm=float("nan")), dict(admit_rssi_dbm=float("inf")), dict(admit_rssi_dbm=-float("inf")), dict(admit_rssi_dbm=-300.5),
             dict(timeout_us=-1), dict(timeout_us=0), dict(timeout_us=1 << 62), dict(timeout_us=(1 << 62) + 1), dict(min_heard=0),
             dict(min_heard=1 << 31), dict(min_heard=(1 << 31) + 1), dict(evict_cost=0), dict(evict_cost=1), dict(evict_cost=127), dict(evict_cost=128),
             dict(evict_cost=(1 << 32) - 1), dict(require_delivered=0), dict(require_delivered=2), dict(require_delivered=-1), dict(reserved=1)]
    for kw in cases:
        want = R.valid(dict(R.DEFAULTS, **kw))
        assert (rsa.Engine.nbtable_validate(rsa.Engine.nbtable_params(**kw)) == 0) == want, kw
    assert rsa._lib.lib().rm_nbtable_validate(None) == INVALID
    # the host functions' own refusals: nothing changes
    peer = np.full((3, 2), -1, dtype=np.int32)
    stats = np.zeros((3, 2), dtype=rsa._lib.LINK_STATS_DTYPE)
    res = host_result(R.Result([0], 0, [0, 1], [1], [2], [-50.0]))
    for call in (lambda: rsa.Engine.nbtable_from_result(res, [0], [0], peer, stats, p, -1),
                 lambda: rsa.Engine.nbtable_from_result(res, [0], [0], peer, stats, p, 0, pin=[0, 3, -1]),
                 lambda: rsa.Engine.nbtable_from_result(res, [0], [0], peer, stats, rsa.Engine.nbtable_params(evict_cost=5), 0),
                 lambda: rsa.Engine.nbtable_expire_tables(peer, stats, p, -1), lambda: rsa.Engine.nbtable_expire_tables(peer, stats, p, 0, pin=[3, 0, 0]),
                 lambda: rsa.Engine.nbtable_expire_tables(np.full((3, 3), -1, dtype=np.int32), np.zeros((3, 3), dtype=stats.dtype), p, 0)):
        with pytest.raises(rsa.RadioMediumError) as e:
            call()
        assert e.value.code == INVALID
    assert (peer == -1).all() and not stats["heard"].any()


def test_host_rule_under_sanitizers(rsa, tmp_path):
    """tests/cpp/nbtable_host_san_test.cpp with rm_api_nbtable.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "nbtable_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_nbtable.cpp"), os.path.join(ROOT, "tests", "cpp", "nbtable_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
