"""CPU tier of the forwarding queues.  1. the REFERENCE (tests/fwd_ref.py over ticks the oracle evaluates)
plays every scene of tests/test_gpu_fwd.py end to end and is held to the conditions that make those scenes worth running: if a scene
misses one, the scene changes, not the condition.  Both identities and the invariant are asserted after every step (Driver.after).
2. the library's pure host functions rm_fwd_backoff / rm_fwd_validate / rm_fwd_defaults against that reference.  3. the same
functions and the host validation paths in a stand-alone program under the host sanitizers (tests/cpp/fwd_host_san_test.cpp)."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fwd_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(*a, **kw):
    return F.Driver(*a, **kw)


# ---- 1. the scenes on the reference -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [40, 70])
def test_line_every_packet_arrives_with_its_distance(O, n):
    d = F.scene_line(_make, n)
    t, c = d.ref.totals(), d.ref.c
    assert t["generated"] == t["arrived"] == n and t["in_flight"] == 0
    assert c["arrived"] == [1] * n and c["hops_sum"] == list(range(n))
    assert d.log["steps"] >= n - 1 and sum(c["attempts"]) == t["hops_sum"] + sum(c["failed"])
    assert t["hops_sum"] == n * (n - 1) // 2


@pytest.mark.parametrize("leaves", [64, 65, 129, 257])
def test_hub_sink(O, leaves):
    d = F.scene_hub_sink(_make, leaves)
    t, c = d.ref.totals(), d.ref.c
    assert t["arrived"] == leaves and t["hops_sum"] == leaves and t["in_flight"] == 0
    assert c["acked"][:leaves] == [1] * leaves and c["arrived"][:leaves] == [1] * leaves
    assert t["latency_us_sum"] == leaves * (F.TICK * 0 + 100 + F.AIR - 10)


@pytest.mark.parametrize("arrivals, preload, accepted", [(16, 0, True), (17, 0, False), (15, 1, True), (16, 1, False)])
def test_hub_relay_accepts_all_or_none(O, arrivals, preload, accepted):
    d = F.scene_hub_relay(_make, arrivals, preload)
    c, hub = d.ref.c, 20
    assert c["rejected"][hub] == (0 if accepted else arrivals)
    assert sum(c["acked"][:20]) == (arrivals if accepted else 0) and sum(c["failed"][:20]) == (0 if accepted else arrivals)
    # the hub's own frame reached the sink behind it, and its pop made no room
    assert c["acked"][hub] == preload and len(d.ref.q[hub]) == (arrivals if accepted else 0)
    assert c["queue_max"][hub] == (preload + arrivals if accepted else preload)


LATTICE_CASES = [(0, 0, 0), (3, 0, 0), (0, 3, 5), (3, 3, 5)]


@pytest.mark.parametrize("retries, min_be, max_be", LATTICE_CASES)
def test_lattice(O, retries, min_be, max_be):
    d = F.scene_lattice(_make, retries, min_be, max_be)
    t, c = d.ref.totals(), d.ref.c
    assert t["generated"] > 30 and t["arrived"] >= 5 and t["dropped_retries"] >= 1 and sum(c["failed"]) > 30
    assert t["hops_sum"] > 2 * t["arrived"]                      # (multi-hop arrivals)
    if retries:
        assert sum(c["failed"]) > t["dropped_retries"]           # (a retry got through or waits)
    ends = [r % F.TICK == 100 + F.AIR for r in d.ref.ready if r]
    if max_be == 0 or retries == 0:                              # r is always 0, or nobody backs off: ready_us is a frame's end
        assert all(ends)
    else:                                                        # the unit is 1000 us: a drawn backoff shows in ready_us
        assert not all(ends)


def test_gated_defers_with_the_candidate_list_and_not_without(O):
    a = F.scene_lattice(_make, 3, 3, 5, steps=120, cca=(128, -88.0), cand=True)
    b = F.scene_lattice(_make, 3, 3, 5, steps=120, cca=(128, -88.0), cand=False)
    assert a.log["deferred_lists"] >= 1 and b.log["deferred_lists"] >= 1
    assert sum(a.ref.c["deferred"]) >= 1 and sum(b.ref.c["deferred"]) == 0
    assert a.ref.totals()["arrived"] > 0 and b.ref.totals()["arrived"] > 0


@pytest.mark.parametrize("n", [1025, 4097])
def test_big_source_lists(O, n):
    d = F.scene_big(_make, n)
    m = d.asked[2][0]
    assert m >= 2 * ((n - 1) // 256) and d.asked == [(0, 7), (1, 7), (m, m + 1), (m, m), (m, m - 1), (m, 1), (m, m), (1, m)]
    assert d.log["truncated"] >= 2
    lst = d.loaded
    # sendable nodes on both sides of every 256 (and so 1024) boundary
    assert all(b in lst for b in range(256, n - 1, 256)) and all(b - 1 in lst for b in range(256, n - 1, 256))
    assert d.ref.totals()["dropped_full"] == 0 and sum(d.ref.c["attempts"]) >= 1


def test_reroute(O):
    d = F.scene_reroute(_make)
    t, c = d.ref.totals(), d.ref.c
    assert t["dropped_no_route"] == 3 and c["dropped"][5] == 3 and c["lost"][5] == 3
    assert c["arrived"][3] == 2 and c["latency_us_sum"][3] == 2 * 777 and c["hops_sum"][3] == 0
    assert t["dropped_ttl"] == 2 and c["lost"][6] == 1 and c["lost"][7] == 1 and t["in_flight"] == 0
    assert d.ref.next[5] == F.NO_ROUTE and d.ref.next[3] == F.SINK and d.ref.next[0] == F.SINK


def test_batch_equals_lone_ticks_and_holds_a_stray(O):
    a, b = F.scene_batch(_make, True), F.scene_batch(_make, False)
    assert a.ref.table() == b.ref.table() and a.ref.totals() == b.ref.totals() and a.ref.queues() == b.ref.queues()
    assert a.ref.totals()["stray"] >= 1 and a.ref.tries[2] > 0        # (node 2, listed again while in backoff)
    assert a.ref.totals()["arrived"] > 0


def test_the_scenes_together_hit_every_case(O):
    runs = [F.scene_hub_relay(_make, 17, 0), F.scene_reroute(_make), F.scene_lattice(_make, 0, 3, 5, steps=60),
            F.scene_lattice(_make, 3, 3, 5, steps=60, cca=(128, -88.0)), F.scene_batch(_make, True), F.scene_big(_make, 1025)]
    tot = {k: sum(r.ref.totals()[k] for r in runs) for k in F.TOTALS}
    assert sum(sum(r.ref.c["rejected"]) for r in runs) >= 1 and tot["dropped_retries"] >= 1 and tot["dropped_ttl"] >= 1
    assert sum(sum(r.ref.c["deferred"]) for r in runs) >= 1 and tot["stray"] >= 1 and sum(r.log["truncated"] for r in runs) >= 1


def test_a_lost_slot_is_skipped():
    s = F.State(4)
    s.set_next([-1, 0, 1, 2], [0], 0)
    s.inject([1, 2, 3], 0)
    before = (s.table(), s.queues())
    s.advance(F.Result([1, 2, 3], 0, 100, [0, 0, 0, 0], [], [], lost=True))
    assert (s.table(), s.queues()) == before and s.totals()["skipped_slots"] == 1


# ---- 2. the pure host functions through the binding -------------------------------------------------------------------------------

def _params(rsa, **kw):
    from radio_sim_amd import _lib
    p = _lib.FwdParams()
    _lib.lib().rm_fwd_defaults(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_and_validate_against_the_reference(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    p = _params(rsa)
    assert {k: getattr(p, k) for k in F.DEFAULTS} == F.DEFAULTS
    assert L.rm_fwd_validate(C.byref(p)) == 0 and L.rm_fwd_validate(None) == -1
    grid = dict(queue_slots=(0, 1, 2, 3, 4, 8, 15, 16, 32, -1), max_retries=(-1, 0, 15, 16), min_be=(-1, 0, 3, 8, 9), max_be=(-1, 0, 2, 8, 9),
                max_hops=(0, 1, 255, 256), backoff_unit_us=(-1, 0, 1 << 32, (1 << 32) + 1), reserved=(0, 1))
    for k, values in grid.items():
        for v in values:
            for extra in ({}, {"min_be": 0, "max_be": 0}, {"min_be": 8, "max_be": 8}):
                kw = dict(extra, **{k: v})
                want = F.valid(dict(F.DEFAULTS, **kw))
                assert (L.rm_fwd_validate(C.byref(_params(rsa, **kw))) == 0) == want, kw


def test_backoff_against_the_reference(rsa):
    from radio_sim_amd import _lib
    L = _lib.lib()
    d = C.c_int64(-7)
    for seed, (lo, hi), unit in itertools.product((0, 1, 0xDEADBEEFCAFEF00D, (1 << 64) - 1), ((0, 0), (0, 8), (3, 5), (8, 8), (1, 1)), (0, 320, 1 << 32)):
        p = _params(rsa, seed=seed, min_be=lo, max_be=hi, backoff_unit_us=unit)
        ref = dict(F.DEFAULTS, seed=seed, min_be=lo, max_be=hi, backoff_unit_us=unit)
        for node, start, tries in itertools.product((0, 1, 77, (1 << 31) - 1), (0, 1, 4356, (1 << 62) + 5), (1, 2, 3, 9, 16)):
            assert L.rm_fwd_backoff(C.byref(p), node, start, tries, C.byref(d)) == 0
            r = F.backoff_factor(ref, node, start, tries)
            assert r < (1 << min(lo + tries - 1, hi)) and d.value == r * unit, (seed, lo, hi, unit, node, start, tries)
    p = _params(rsa)
    for bad in ((-1, 0, 1), (0, -1, 1), (0, 0, 0)):
        d.value = -7
        assert L.rm_fwd_backoff(C.byref(p), *bad, C.byref(d)) == -1 and d.value == -7
    assert L.rm_fwd_backoff(C.byref(_params(rsa, queue_slots=3)), 0, 0, 1, C.byref(d)) == -1
    assert L.rm_fwd_backoff(C.byref(p), 0, 0, 1, None) == -1
    # the draws spread: over 4096 nodes at BE 5 every factor 0 .. 31 occurs
    ref = dict(F.DEFAULTS, min_be=5, max_be=5)
    assert {F.backoff_factor(ref, j, 1000, 1) for j in range(4096)} == set(range(32))


# ---- 3. the host functions under the host sanitizers, in a stand-alone program -----------------------------------------------------

def test_host_functions_under_sanitizers(rsa, tmp_path):
    """tests/cpp/fwd_host_san_test.cpp with rm_api_fwd.cpp compiled beside it under -fsanitize=address,undefined (host code only:
    the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "fwd_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_fwd.cpp"), os.path.join(ROOT, "tests", "cpp", "fwd_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
