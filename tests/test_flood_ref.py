"""CPU tier of the dissemination floods.  1. the REFERENCE (tests/flood_ref.py over ticks the oracle
evaluates) plays every scene of tests/test_gpu_flood.py end to end and is held to the conditions that make those scenes worth
running: if a scene misses one, the scene changes, not the condition.  The identities are asserted after every step (Driver.after).
2. the library's pure host functions rm_flood_fire / rm_flood_validate / rm_flood_defaults against that reference.  3. the same
functions and the host validation paths in a stand-alone program under the host sanitizers (tests/cpp/flood_host_san_test.cpp)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

import flood_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(*a, **kw):
    return F.Driver(*a, **kw)


# ---- 1. the scenes on the reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [40, 70])
def test_line_hop_is_the_distance(O, n):
    d = F.scene_line(_make, n)
    r, t = d.ref, d.ref.totals()
    assert t["covered"] == n and t["seeds"] == 1 and t["max_hop"] == n - 1
    assert r.hop == list(range(n)) and r.parent == list(range(-1, n - 1))
    assert all(a < b for a, b in zip(r.first, r.first[1:])) and t["last_first_us"] == r.first[-1]


@pytest.mark.parametrize("n", [64, 65])
def test_clique_suppression(O, n):
    a, b = F.scene_clique(_make, n, 1), F.scene_clique(_make, n, 0)
    assert a.covered_after_first == n and b.covered_after_first == n
    ta, tb = a.ref.totals(), b.ref.totals()
    assert ta["suppressed"] > 0 and ta["sent"] * 8 < n and ta["sent"] >= 3          # (the seed's frame and one per later interval at least)
    assert tb["suppressed"] == 0 and tb["sent"] == 3 * n
    assert all(m == 3 for m in a.ref.m) and all(f == -1 for f in a.ref.fire)


def test_lattice_ties_collisions_and_sleepers(O):
    d = F.scene_lattice(_make)
    t = d.ref.totals()
    assert d.log["ties"] >= 1 and d.log["collided"] >= 1 and d.log["missed"] >= 1
    assert 100 < t["covered"] < d.nd.n and t["suppressed"] > 0 and t["max_hop"] >= 8


def test_foreign_frames_change_verdicts_and_carry_nothing(O):
    a, b = F.scene_foreign(_make, True), F.scene_foreign(_make, False)
    assert a.log["foreign_delivered"] >= 1 and a.log["foreign_collided"] >= 1 and b.log["foreign_delivered"] == 0
    assert a.ref.first[5] > b.ref.first[5] > 0 and a.ref.first[:5] == b.ref.first[:5]
    assert a.ref.first[6:] == [-1] * 6 and a.ref.cnt["heard"][7:] == [0] * 5 and a.ref.cnt["sent"][6:] == [0] * 6


def test_gated_defers_with_the_candidate_list_and_not_without(O):
    a, b = F.scene_gated(_make, True), F.scene_gated(_make, False)
    assert a.log["deferred_lists"] >= 1 and b.log["deferred_lists"] >= 1
    assert sum(a.ref.cnt["deferred"]) >= 1 and sum(b.ref.cnt["deferred"]) == 0
    assert any(x > 0 and s > 0 for x, s in zip(a.ref.cnt["deferred"], a.ref.cnt["sent"]))       # (deferred, still due, sent later)


@pytest.mark.parametrize("n", [1025, 4097])
def test_big_many_due_at_once(O, n):
    d = F.scene_big(_make, n)
    m = d.n_seeds
    assert m > 256 and d.asked == [0, m, m, m, m, m] and d.log["truncated"] >= 2
    t = d.ref.totals()
    assert t["seeds"] == m and t["covered"] > m and t["suppressed"] > 100 and t["sent"] == 72


def test_batch_equals_lone_ticks_and_holds_strays(O):
    a, b = F.scene_batch(_make, True), F.scene_batch(_make, False)
    assert a.ref.table() == b.ref.table() and a.ref.totals() == b.ref.totals()
    t = a.ref.totals()
    assert t["stray"] >= 2 and t["covered"] > t["seeds"] and a.ref.cnt["sent"][9] == 0 and a.ref.cnt["sent"][2] == 1
    assert a.log["ties"] >= 1


def test_limits(O):
    d = F.scene_max_hops(_make)
    assert d.ref.first[3:] == [-1] * 3 and min(d.ref.first[:3]) >= 0 and d.ref.cnt["heard"][3] >= 1
    d = F.scene_one_interval(_make)
    r = d.ref
    assert all(s + q == 1 for s, q in zip(r.cnt["sent"], r.cnt["suppressed"])) and r.fire == [-1] * r.n and r.start == [-1] * r.n
    assert sum(r.cnt["suppressed"]) >= 1
    d = F.scene_capacity(_make)
    assert d.unchanged and d.ref.totals()["skipped_slots"] == 1 and d.ref.totals()["covered"] == d.nd.n


def test_seed_rules():
    s = F.State(5)
    s.seed([1, 1, -1, 5, 9, 3], 10)
    assert s.totals()["seeds"] == 2 and s.first == [-1, 10, -1, 10, -1]
    s.seed([1, 2], 20)
    assert s.first == [-1, 10, 20, 10, -1] and s.totals()["last_first_us"] == 20 and s.hop == [-1, 0, 0, 0, -1]
    s.check()


def test_a_suppressed_node_is_not_listed_even_if_due_again():
    s = F.State(2, imin_us=2, doublings=0, max_intervals=4, redundancy=1)
    s.seed([0, 1], 0)
    s.c[0] = 1
    lst, count = s.sources(1000, 4)
    assert (lst, count) == ([1, -1, -1, -1], 1) and s.m[0] == 1 and s.fire[0] <= 1000 and s.cnt["suppressed"][0] == 1
    assert s.sources(1000, 4)[0][:2] == [0, 1]


# ---- 2. the pure host functions through the binding -------------------------------------------------------------------------------

def _params(rsa, **kw):
    from radio_sim_amd import _lib
    p = _lib.FloodParams()
    _lib.lib().rm_flood_defaults(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_and_validate_against_the_reference(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    p = _params(rsa)
    assert {k: getattr(p, k) for k in F.DEFAULTS} == F.DEFAULTS
    assert L.rm_flood_validate(C.byref(p)) == 0 and L.rm_flood_validate(None) == -1
    grid = dict(imin_us=(-1, 0, 1, 2, 8000, 1 << 32, (1 << 32) + 1), doublings=(-1, 0, 16, 17), max_intervals=(0, 1, 64, 65),
                redundancy=(-1, 0, 255, 256), max_hops=(0, 1, 65535, 65536))
    for k, values in grid.items():
        for v in values:
            assert (L.rm_flood_validate(C.byref(_params(rsa, **{k: v}))) == 0) == F.valid(dict(F.DEFAULTS, **{k: v})), (k, v)
    assert rsa.Engine.flood_validate(rsa.Engine.flood_params(redundancy=7)) == 0


def test_fire_against_the_reference(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    s, f = C.c_int64(-7), C.c_int64(-7)
    for seed, imin, D in itertools.product((0, 1, 0xDEADBEEFCAFEF00D, (1 << 64) - 1), (2, 3, 8000, 1 << 32), (0, 4, 16)):
        p = _params(rsa, seed=seed, imin_us=imin, doublings=D, max_intervals=64)
        ref = dict(F.DEFAULTS, seed=seed, imin_us=imin, doublings=D, max_intervals=64)
        for node, first, m in itertools.product((0, 1, 77, (1 << 31) - 1), (0, 1, 4356, 1 << 40), (0, 1, 3, 4, 5, 17, 63, 64)):
            assert L.rm_flood_fire(C.byref(p), node, first, m, C.byref(s), C.byref(f)) == 0
            assert (s.value, f.value) == F.fire(ref, node, first, m), (seed, imin, D, node, first, m)
            if m < 64:
                length = imin << min(m, D)
                assert s.value + length // 2 <= f.value < s.value + length
    p = _params(rsa)
    for bad in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 9)):
        s.value = -7
        assert L.rm_flood_fire(C.byref(p), *bad, C.byref(s), C.byref(f)) == -1 and s.value == -7
    assert L.rm_flood_fire(C.byref(_params(rsa, imin_us=1)), 0, 0, 0, C.byref(s), C.byref(f)) == -1
    assert L.rm_flood_fire(C.byref(p), 0, 0, 0, None, C.byref(f)) == -1
    assert rsa.Engine.flood_fire(p, 3, 100, 8) == (-1, -1) and rsa.Engine.flood_fire(p, 3, 100, 2) == F.fire(F.DEFAULTS, 3, 100, 2)
    # the draws spread over the second half of the interval
    r = [F.fire(F.DEFAULTS, j, 0, 0)[1] for j in range(4096)]
    assert min(r) < 4000 + 40 and max(r) >= 8000 - 40 and len(set(r)) > 2000


# ---- 3. the host functions under the host sanitizers, in a stand-alone program -----------------------------------------------------

def test_host_functions_under_sanitizers(rsa, tmp_path):
    """tests/cpp/flood_host_san_test.cpp with rm_api_flood.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "flood_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_flood.cpp"), os.path.join(ROOT, "tests", "cpp", "flood_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
