"""Watched-link statistics without a device: 1. the REFERENCE (tests/linkstats_ref.py over the oracle)
is held to the conditions that make the scenes of tests/test_gpu_linkstats.py worth running -- if a scene misses one, the scene
changes, not the condition; 2. the library's pure host functions rm_linkstats_q8 and rm_linkstats_validate against that reference;
3. the same functions in a stand-alone program under the host sanitizers (tests/cpp/linkstats_host_san_test.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import errmodel_ref as R
import linkstats_ref as K
import listen_ref as LR
import stats_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1


# ---- 1. the reference alone --------------------------------------------------------------------------------------------------

def test_q8_known_answers():
    assert K.q8(0.0) == 0 and K.q8(-0.0) == 0 and K.q8(1.0) == 256 and K.q8(-1.0) == -256 and K.q8(-91.5) == -23424
    for m in (-3, -2, -1, 0, 1, 2, 1000, -1000):
        assert K.q8((m + 0.5) / 256.0) == m + 1   # ties go up, for negative values as well
    assert K.q8(2147483647.99) == 549755813885 and K.q8(-2147483647.99) == -549755813885
    for x in (2147483648.0, -2147483648.0, 1e300, np.nan, np.inf, -np.inf):
        assert K.q8(x) == 0
    assert K.q8(np.array([1.0, np.nan, -2.0])).tolist() == [256, 0, -512]


def test_table_by_hand():
    """three nodes' worth of hand-made links: matched and unmatched, the keep / clear rule, reset"""
    class Res:
        pass
    w = Res()
    w.pkt = np.array([0, 0, 1, 1, 2], dtype=np.int32)
    w.dst = np.array([1, 2, 0, 2, 1], dtype=np.int32)
    w.verdict = np.array([R.O.DELIVERED, R.O.INTERFERED, R.O.DELIVERED, R.O.DELIVERED, R.O.DELIVERED], dtype=np.uint8)
    w.rssi = np.array([-50.0, -60.5, -70.0, -80.0, np.nan])
    w.sinr = np.array([10.0, 1.0, 5.0, 6.0, 7.0])
    new = np.zeros(3, dtype=R.O.PACKET_DTYPE)
    new["src"] = [0, 1, -1]          # the third frame is padding: its link counts nowhere
    new["start_us"] = [100, 50, 70]
    t = K.Table(4, 2)
    t.watch(None, [[-1, -1], [3, 0], [1, 0], [-1, -1]])
    assert t.add(new, w) == (3, 2)   # 0 -> 1, 0 -> 2, 1 -> 2 match; 1 -> 0 is not watched; the padding's link has no source
    e = t.t[1, 1]
    assert e.tolist() == (1, 1, -12800, 2560, 100, 100)
    assert t.t[2, 0].tolist() == (1, 1, -20480, 1536, 50, 50)
    assert t.t[2, 1].tolist() == (1, 0, -15488, 256, 100, 100)
    assert t.t[0, 0].tolist() == K.CLEARED and t.t[1, 0].tolist() == K.CLEARED
    new["start_us"] = [30, 500, 70]
    t.add(new, w, sinr=False)
    assert t.t[2, 0].tolist() == (2, 2, -40960, 1536, 50, 500) and t.t[1, 1].tolist() == (2, 2, -25600, 2560, 30, 100)
    # node 2 swaps the peer of slot 0 and keeps slot 1; node 1 is not listed
    t.watch([2], [[3, 0]])
    assert t.t[2, 0].tolist() == K.CLEARED and t.t[2, 1]["heard"] == 2 and t.t[1, 1]["heard"] == 2
    assert t.peer.tolist() == [[-1, -1], [3, 0], [3, 0], [-1, -1]]
    assert t.totals() == {"ticks_counted": 2, "ticks_skipped": 0}
    t.reset()
    assert (t.t == np.array(K.CLEARED, dtype=K.DTYPE)).all() and t.peer[2].tolist() == [3, 0] and t.totals()["ticks_counted"] == 0


def _runs(name):
    nd, lists, starts, air, sched, _, runs, _ = LR.scene(name)
    return nd, runs


THRESHOLDS = {   # (scene, K): matched, unmatched, entries with heard >= 2, entries with 0 < delivered < heard (None: not asked)
    ("batch", 4): (10000, 10000, 400, 80),
    ("batch_overlap", 4): (10000, 10000, 1000, 200),
    ("batch", 1): (3000, None, 150, None),
    ("batch", 8): (20000, 10000, None, None),
}


@pytest.mark.parametrize("name,k", sorted(THRESHOLDS))
def test_batch_scenes_hold_the_thresholds(name, k):
    nd, runs = _runs(name)
    run = runs[None]
    pairs = list(zip(run.new, run.res))
    assert sum(w.count for w in run.res) == {"batch": 39130, "batch_overlap": 38659}[name]
    t, matched, unmatched = K.table_of(nd.n, k, K.rows_first_heard(nd.n, k, pairs), pairs, run.after)
    c = K.conditions(t, matched, unmatched)
    print(name, k, c)
    want = THRESHOLDS[(name, k)]
    for got, least in zip((c["matched"], c["unmatched"], c["heard2"], c["partly"]), want):
        assert least is None or got >= least, (c, want)


@pytest.mark.parametrize("name", ["lone", "serial", "batch", "batch_overlap", "udgm", "null"])
@pytest.mark.parametrize("k", K.KS)
def test_every_slot_position_is_hit(name, k):
    if name in ("udgm", "null"):
        scene = S.scene_udgm() if name == "udgm" else S.scene_null()
        nd, pairs = scene[0], [(scene[3], S.oracle_tick(scene))]
        verdicts = None
    else:
        nd, runs = _runs(name)
        pairs, verdicts = list(zip(runs[None].new, runs[None].res)), runs[None].after
    rows = K.rows_first_heard(nd.n, k, pairs)
    assert K.valid(nd.n, k, rows)
    t, matched, unmatched = K.table_of(nd.n, k, rows, pairs, verdicts, sinr=name not in ("udgm", "null"))
    c = K.conditions(t, matched, unmatched)
    assert all(v >= 1 for v in c["slots_hit"]), c
    assert matched == int(t.t["heard"].sum()) and matched + unmatched == sum(w.count for _, w in pairs)
    # untouched entries stay cleared
    idle = t.t["heard"] == 0
    assert (t.t["first_start_us"][idle] == K.I64_MAX).all() and (t.t["last_start_us"][idle] == K.I64_MIN).all()
    assert (t.t["first_start_us"][~idle] <= t.t["last_start_us"][~idle]).all()


# ---- 2. the library's pure host functions against the reference ------------------------------------------------------------------

def test_rm_linkstats_q8_equals_the_reference(rsa):
    from radio_sim_amd import _lib
    q8 = _lib.lib().rm_linkstats_q8
    edges = [(m + 0.5) / 256.0 for m in (-100000, -257, -256, -3, -2, -1, 0, 1, 2, 255, 256, 100000)]
    edges += [-0.0, 0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 2147483647.99, -2147483647.99, 2147483648.0, -2147483648.0,
              np.nextafter(2147483648.0, 0.0), np.nextafter(-2147483648.0, 0.0), 1e300, -1e300, np.nan, np.inf, -np.inf, -91.0, -54.321, 17.77]
    for x in edges:
        assert q8(float(x)) == int(K.q8(x)), x
    assert q8(0.5 / 256.0) == 1 and q8(-0.5 / 256.0) == 0 and q8(-1.5 / 256.0) == -1
    rng = np.random.default_rng(14)
    xs = np.concatenate([rng.uniform(-120.0, 60.0, 4000), rng.integers(-40000, 40000, 2000) / 512.0, rng.uniform(-3e9, 3e9, 500)])
    want = K.q8(xs)
    assert (want == 0).sum() > 50 and (want < 0).any() and (want > 0).any()
    for x, w in zip(xs.tolist(), want.tolist()):
        assert q8(x) == w, x


def _validate(n_nodes, k, rows, nodes=None, n=None):
    from radio_sim_amd import _lib
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    idx = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
    if n is None:
        n = len(idx) if idx is not None else len(rows) // max(k, 1)
    return _lib.lib().rm_linkstats_validate(n_nodes, k, None if idx is None else idx.ctypes.data, n, rows.ctypes.data)


def test_rm_linkstats_validate_accepts_and_refuses_what_the_rule_says(rsa):
    n = 10
    good = [[1, 2, -1, 9], [-1, -1, -1, -1], [4, 3, 1, 0]]
    nodes = [0, 5, 2]
    assert K.valid(n, 4, good, nodes) and _validate(n, 4, good, nodes) == OK
    cases = {
        "own node as peer": ([[1, 2, 0, 9], good[1], good[2]], nodes, 4),
        "a repeated peer in a row": ([good[0], good[1], [4, 3, 1, 4]], nodes, 4),
        "a repeated node": (good, [0, 5, 0], 4),
        "a peer out of range": ([[1, 2, -1, 10], good[1], good[2]], nodes, 4),
        "a peer below -1": ([[1, -2, -1, 9], good[1], good[2]], nodes, 4),
        "a node out of range": (good, [0, 10, 2], 4),
        "a negative node": (good, [0, -1, 2], 4),
        "K = 3": ([[1, 2, 3]], [0], 3),
        "K = 0": ([[1]], [0], 0),
        "K = 16": ([list(range(1, 17))], [0], 16),
    }
    for what, (rows, idx, k) in cases.items():
        assert not K.valid(n, k, rows, idx), what
        assert _validate(n, k, rows, idx) == INVALID, what
    # nodes == NULL: all nodes, n has to be the node count
    whole = K.rows_first_heard(n, 2, [])   # every slot empty
    whole[:, 0] = (np.arange(n) + 1) % n
    assert K.valid(n, 2, whole) and _validate(n, 2, whole) == OK
    assert not K.valid(n, 2, whole[:-1]) and _validate(n, 2, whole[:-1]) == INVALID
    assert _validate(n + 1, 2, whole) == INVALID
    whole[3, 1] = 3
    assert not K.valid(n, 2, whole) and _validate(n, 2, whole) == INVALID
    # NULL peers with a count, a negative count; an empty list is fine
    from radio_sim_amd import _lib
    L = _lib.lib()
    idx = np.array(nodes, dtype=np.int32)
    assert L.rm_linkstats_validate(n, 4, idx.ctypes.data, 3, None) == INVALID
    assert L.rm_linkstats_validate(n, 4, idx.ctypes.data, -1, None) == INVALID
    assert L.rm_linkstats_validate(n, 4, idx.ctypes.data, 0, None) == OK
    # every K the rule names, and the scenes' own rows
    for k in K.KS:
        nd, runs = _runs("lone")
        rows = K.rows_first_heard(nd.n, k, list(zip(runs[None].new, runs[None].res)))
        assert _validate(nd.n, k, rows) == OK


# ---- 3. the host functions under the host sanitizers, in a stand-alone program -----------------------------------------------------

def test_host_functions_under_sanitizers(rsa, tmp_path):
    """tests/cpp/linkstats_host_san_test.cpp with rm_api_linkstats.cpp compiled beside it under -fsanitize=address,undefined (host
    code only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "linkstats_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_linkstats.cpp"), os.path.join(ROOT, "tests", "cpp", "linkstats_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
