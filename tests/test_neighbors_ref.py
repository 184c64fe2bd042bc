"""The neighbour query's reference (tests/neighbors_ref.py) held to the scene conditions the GPU tests
rely on, the pure host function rm_neighbors_from_result against it, and the ABI's new names.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import neighbors_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", N.RICH)
def test_scene_conditions(O, name):
    """every rich scene: degrees 0, below K, K and above K for every K of the tests; a disabled, an rxprob = 0 and an other-channel
    receiver inside the source's reach and in no row; unequal txpower that makes a HEARS row differ from the HEARD_BY row; without
    shadowing an exact rssi tie decided by node index.  (The scenes of 1, 2 and 3 nodes cannot hold these.)"""
    nd, params, found = N.scene(name)
    sp = N.special(nd)
    S, A, B = sp["S"], sp["A"], sp["B"]
    assert len(set(nd.txpower.tolist())) >= 3
    for d in (N.HEARD_BY, N.HEARS):
        deg = np.array([len(found[d][j]) for j in range(nd.n)])
        assert deg[sp["LONE"]] == 0
        for K in N.KS:
            assert (deg == 0).any() and ((deg > 0) & (deg < K)).any() == (K > 1) and (deg == K).any() and (deg > K).any(), (name, d, K, np.bincount(deg))
    by = {f[1]: f[0] for f in found[N.HEARD_BY][S]}
    for gone in ("OFF", "DEAF", "OTHER"):
        assert sp[gone] not in by, gone
        # ... though inside reach: the same place hears S once the reason is taken away
    plain = N.O.NodeTable(nd.n)
    for f in ("x", "y", "z", "txpower"):
        setattr(plain, f, np.array(getattr(nd, f)))
    reach = {f[1] for f in N.links(plain, params, N.HEARD_BY, [S])[S]}
    assert {sp["OFF"], sp["DEAF"], sp["OTHER"]} <= reach
    # S transmits to the disabled and the deaf node's place in vain, but THEY are heard by S: enabled_s plays no part
    hears = {f[1] for f in found[N.HEARS][S]}
    assert sp["OFF"] in hears and sp["DEAF"] in hears and sp["OTHER"] not in hears
    differ = [j for j in range(nd.n) if N.rank(found[N.HEARD_BY][j], 16)[0] != N.rank(found[N.HEARS][j], 16)[0]]
    assert differ, "no node's HEARS row differs from its HEARD_BY row"
    if params["ld_sigma_db"] == 0.0:
        assert sp["LOUD"] in hears and sp["LOUD"] not in by
        assert A in by and B in by and N.bits([by[A]])[0] == N.bits([by[B]])[0]
        peer = N.rank(found[N.HEARD_BY][S], 16)[0]
        assert peer.index(A) + 1 == peer.index(B)
    else:
        assert params["ld_clip"] == 3.0
        assert A in by and B in by and N.bits([by[A]])[0] != N.bits([by[B]])[0]


def test_rank_is_the_rule():
    """descending rssi, ties (-0.0 == +0.0 among them) by node index, NaN is no link, the padding"""
    found = [(-80.0, 9), (-70.0, 4), (-80.0, 2), (float("nan"), 1), (0.0, 8), (-0.0, 7), (-70.0, 5)]
    peer, rb, deg = N.rank(found, 8)
    assert peer == [7, 8, 4, 5, 2, 9, -1, -1] and deg == 6
    assert rb[6] == rb[7] == N.NAN_BITS and rb[0] == int(N.bits([-0.0])[0]) and rb[1] == 0
    assert N.rank(found, 2)[0] == [7, 8] and N.rank([], 3) == ([-1, -1, -1], [N.NAN_BITS] * 3, 0)


@pytest.mark.parametrize("name", ["one", "three", "n65", "n300_shadow"])
def test_from_result_against_the_reference(rsa, O, name):
    """rm_neighbors_from_result over a tick of distinct sources (each alone in its channel as far as heard links go: the medium
    without SINR evaluates packets independently) gives the HEARD_BY rows of the sources"""
    nd, params, found = N.scene(name)
    srcs = np.arange(nd.n, dtype=np.int32)[::-1].copy()   # (any order of distinct sources)
    res = N.host_result(nd, params, srcs)
    for K in N.KS:
        want = N.rows(nd, params, N.HEARD_BY, K, srcs, found[N.HEARD_BY])
        N.same(rsa.Engine.neighbors_from_result(res, K), want, "%s K=%d" % (name, K))
        N.same(rsa.Engine.neighbors_from_result(res, K, fields=()), want, "%s K=%d, peer alone" % (name, K))
    part = rsa.Engine.neighbors_from_result(res, 4, n_pkt=min(2, nd.n))
    N.same(part, tuple(a[:min(2, nd.n)] for a in N.rows(nd, params, N.HEARD_BY, 4, srcs, found[N.HEARD_BY])), name + ": the first packets")


def test_from_result_refusals(rsa, O):
    nd, params, _ = N.scene("three")
    res = N.host_result(nd, params, np.arange(3, dtype=np.int32))
    E = rsa.Engine
    for bad in (lambda: E.neighbors_from_result(res, 0), lambda: E.neighbors_from_result(res, 17), lambda: E.neighbors_from_result(res, 4, n_pkt=4),
                lambda: E.neighbors_from_result(res, 4, n_pkt=-1)):
        with pytest.raises(rsa.RadioMediumError) as e:
            bad()
        assert e.value.code == -1
    res.rssi = None   # links, but no rssi column
    assert res.count > 0
    with pytest.raises(rsa.RadioMediumError) as e:
        E.neighbors_from_result(res, 4)
    assert e.value.code == -1


def test_abi_presence(rsa):
    from radio_sim_amd import _lib
    for name in ("rm_neighbors_query_device", "rm_neighbors_query", "rm_neighbors_from_result", "rm_linkstats_watch_device"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    for name in ("neighbors", "neighbors_device", "neighbors_from_result", "linkstats_watch_device"):
        assert callable(getattr(rsa.Engine, name))
    assert (rsa.NB_HEARD_BY, rsa.NB_HEARS, rsa.NB_MAX_K) == (0, 1, 16)
    assert _lib.lib().rm_abi_version() == 5


def test_host_function_under_sanitizers(rsa, tmp_path):
    """tests/cpp/neighbors_host_san_test.cpp with rm_api_neighbors.cpp compiled beside it under -fsanitize=address,undefined (host
    code only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "neighbors_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_neighbors.cpp"), os.path.join(ROOT, "tests", "cpp", "neighbors_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)


def test_two_tick_hears_reference_is_the_one_tick_reference(O):
    """links_hears_large (what the GPU tests of large tables use) against links() for every node of a shadowed scene, and with
    radios off"""
    nd, params, found = N.scene("n300_shadow")
    got = N.links_hears_large(nd, params, np.arange(nd.n))
    for j in range(nd.n):
        assert sorted(got[j]) == sorted(found[N.HEARS][j]), j
    nd2, ask = N.large(300, 13, 70)
    want, got = N.links(nd2, N.PLAIN, N.HEARS, ask), N.links_hears_large(nd2, N.PLAIN, ask)
    assert any(nd2.enabled[f[1]] == 0 for j in ask for f in want[int(j)])     # (a radio that is off is heard all the same)
    for j in ask:
        assert sorted(got[int(j)]) == sorted(want[int(j)]), j
