"""The link estimator without a GPU: the scenes of tests/linkest_ref.py held to the conditions that make
them worth running -- from the reference alone --, and the pure host functions rm_linkest_fold_tables, rm_linkest_validate and
rm_linkest_defaults against the reference, exactly, after every fold of every scene; the identity that lets the measured-route
query read the published table, over every estimate there is; the bounds of the smoothing; and the host rule under sanitizers in
a stand-alone program.

A table of ONE node can show none of the conditions: by E22's rule every slot of its only row is empty (outside the table, or
the node itself).  Its scene is held to exactly that -- nothing but folds and rebases ever happens -- and stays in the GPU tier
for the launch geometry (a single row, a wave with one live lane group)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import linkest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SIZES = [1, 2, 3, 9, 65, 257]
KS = [1, 2, 4, 8]
VARIANTS = [R.params(), R.params(beacon_window=1, data_window=1, beacon_alpha_q8=0, data_alpha_q8=255, max_etx=65535),
            R.params(beacon_window=0), R.params(data_window=0, max_etx=128)]


# ---- the reference alone: every scene shows what it is there for -------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", SIZES)
def test_scene_conditions(n, K):
    seq = R.scene(n, K)
    assert len(seq) >= 20
    ref = R.play(n, K, R.params(), seq)
    t = ref.totals()
    if n == 1:
        assert (ref.entry["peer"] == -1).all() and not ref.entry["etx"].any() and t["folds"] == len(seq)
        assert not any(t[f] for f in R.TOTALS if f != "folds")
        return
    got = R.conditions(ref)
    assert all(got.values()), got
    assert t["data_samples"] >= 1 and ref.log["rebased"] >= 1
    # the identities of the rule
    assert t["estimates"] == int((ref.entry["etx"] != 0).sum())
    for f in ("restarted", "data_samples", "data_unmatched"):
        assert t[f] == int(ref.node[f].sum()), f
    etx = ref.entry["etx"]
    assert ((etx == 0) | ((etx >= 128) & (etx <= 6400))).all()
    assert (ref.pub_peer == ref.entry["peer"]).all() and (ref.pub_stats["heard"] == etx).all()
    assert (ref.pub_stats["delivered"] == np.where(etx != 0, 128, 0)).all()


def test_scenes_hold_the_listed_mutations():
    """over the scenes together: duplicate peers with a data sample in such a row, delivered > heard, counters near 2^40, every kind
    of empty slot, a next hop that is a sink, no route, the node itself"""
    seen = dict.fromkeys(("dup_sample", "more_delivered", "near_2_40", "minus_one", "self", "above", "sink", "no_route", "next_self"), False)
    for n, K in ((9, 4), (65, 8), (257, 2)):
        seq = R.scene(n, K)
        ref = R.play(n, K, R.params(), seq)
        seen["dup_sample"] |= ref.log["data_dup_row"] >= 1
        rows = np.arange(n)[:, None]
        for peer, stats, fwd in seq:
            seen["more_delivered"] |= bool((stats["delivered"] > stats["heard"]).any())
            seen["near_2_40"] |= bool((stats["heard"] > (1 << 40) - 64).any())
            seen["minus_one"] |= bool((peer == -1).any())
            seen["self"] |= bool((peer == rows).any())
            seen["above"] |= bool((peer >= n).any())
            seen["sink"] |= bool((fwd["next"] == -2).any())
            seen["no_route"] |= bool((fwd["next"] == -1).any())
            seen["next_self"] |= bool((fwd["next"] == np.arange(n)).any())
    assert all(seen.values()), seen


# ---- the rule's arithmetic ----------------------------------------------------------------------------------------------------------

def test_published_entry_costs_its_estimate(rsa):
    """E21's entry cost of {heard = etx, delivered = 128} is etx for every etx in 128 .. 65535: in the reference's text for all of
    them, and through rm_etx_link_cost for all of them"""
    P = rsa.Engine.etx_params(min_heard=1, max_link_cost=65535)
    for etx in range(128, 65536):
        assert R.entry_cost(1, 65535, etx, 128) == etx
        assert rsa.Engine.etx_link_cost(P, etx, 128) == etx
    assert rsa.Engine.etx_link_cost(P, 0, 0) is None               # (the cleared entry does not count)
    P128 = rsa.Engine.etx_params(min_heard=128, max_link_cost=65535)
    assert rsa.Engine.etx_link_cost(P128, 128, 128) == 128 and rsa.Engine.etx_link_cost(P128, 65535, 128) == 65535


def test_ewma_bounds():
    """between min(old, s) and max(old, s) for every alpha, so within 128 .. max_etx; old == 0 takes the sample; the dead band"""
    rng = np.random.default_rng(5)
    for a, old, s in zip(rng.integers(0, 256, 200000).tolist(), rng.integers(128, 65536, 200000).tolist(), rng.integers(128, 65536, 200000).tolist()):
        r = R.ewma(a, old, s)
        assert min(old, s) <= r <= max(old, s), (a, old, s, r)
    for a in range(256):
        for old, s in ((128, 65535), (65535, 128), (128, 128), (65535, 65535), (129, 128), (128, 129)):
            assert min(old, s) <= R.ewma(a, old, s) <= max(old, s)
        assert R.ewma(a, 0, 777) == 777
    assert R.ewma(0, 500, 900) == 900 and R.ewma(255, 500, 900) == 502
    # the dead band at alpha 230: from above the estimate stops 4 units over a constant sample, from below 4 units under it
    old = 6400
    for _ in range(400):
        old = R.ewma(230, old, 256)
    assert old == 260
    old = 128
    for _ in range(400):
        old = R.ewma(230, old, 256)
    assert old == 252


def test_sample():
    assert R.sample(6400, 3, 0) == 6400 and R.sample(6400, 3, 3) == 128 and R.sample(6400, 4, 2) == 256
    assert R.sample(6400, 3, 5) == 128 and R.sample(6400, 1000, 1) == 6400 and R.sample(65535, 3, 2) == 192


def test_validate_and_defaults(rsa):
    E = rsa.Engine
    d = E.linkest_params()
    assert {k: getattr(d, k) for k in R.DEFAULTS} == R.DEFAULTS and d.reserved == 0 and E.linkest_validate(d) == 0
    for kw in (dict(beacon_window=0, data_window=0), dict(beacon_window=1 << 31, data_window=1 << 31), dict(beacon_alpha_q8=0, data_alpha_q8=255),
               dict(max_etx=128), dict(max_etx=65535)):
        assert E.linkest_validate(E.linkest_params(**kw)) == 0 and R.valid(R.params(**kw)), kw
    for kw in (dict(beacon_window=(1 << 31) + 1), dict(data_window=(1 << 31) + 1), dict(beacon_alpha_q8=256), dict(data_alpha_q8=256),
               dict(max_etx=127), dict(max_etx=65536), dict(reserved=1)):
        assert E.linkest_validate(E.linkest_params(**kw)) == INVALID and not R.valid(R.params(**kw)), kw
    assert rsa._lib.lib().rm_linkest_validate(None) == INVALID


# ---- the host rule against the reference --------------------------------------------------------------------------------------------

class HostTables:
    """the five tables of rm_linkest_fold_tables in their after-enable state"""

    def __init__(self, rsa, n, K):
        L = rsa._lib
        self.entry = np.zeros((n, K), dtype=L.LINKEST_ENTRY_DTYPE)
        self.entry["peer"] = -1
        self.node = np.zeros(n, dtype=L.LINKEST_NODE_DTYPE)
        self.node["base_next"] = -1
        self.pub_peer = np.full((n, K), -1, dtype=np.int32)
        self.pub_stats = R.cleared_stats((n, K)).astype(L.LINK_STATS_DTYPE)
        self.totals = np.zeros(1, dtype=L.LINKEST_TOTALS_DTYPE)

    def same(self, ref, what):
        R.same(ref, self.entry, self.node, self.pub_peer, self.pub_stats, {k: int(self.totals[k][0]) for k in R.TOTALS}, what)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", SIZES)
def test_host_rule_equals_the_reference(rsa, n, K, variant):
    """after every fold of 20 and more, every table bit for bit; every third fold goes without the forwarding table"""
    p = VARIANTS[variant]
    P = rsa.Engine.linkest_params(**p)
    t = HostTables(rsa, n, K)
    ref = R.Ref(n, K, p)
    for f, (peer, stats, fwd) in enumerate(R.scene(n, K, seed=2 + variant)):
        fw = None if f % 3 == 2 else fwd
        ins = (peer.copy(), stats.copy(), None if fw is None else fw.copy())
        rsa.Engine.linkest_fold_tables(peer, stats, fw, P, t.entry, t.node, t.pub_peer, t.pub_stats, t.totals)
        ref.fold(peer, stats, fw)
        t.same(ref, "n %d K %d variant %d fold %d" % (n, K, variant, f))
        assert ins[0].tobytes() == peer.tobytes() and ins[1].tobytes() == stats.tobytes() and (fw is None or ins[2].tobytes() == fw.tobytes())


def test_host_rule_refusals(rsa):
    E = rsa.Engine
    t = HostTables(rsa, 2, 1)
    peer, stats = np.array([[1], [0]], dtype=np.int32), R.cleared_stats((2, 1))
    bad = E.linkest_params(max_etx=100)
    with pytest.raises(rsa.RadioMediumError) as e:
        E.linkest_fold_tables(peer, stats, None, bad, t.entry, t.node, t.pub_peer, t.pub_stats, t.totals)
    assert e.value.code == INVALID and not t.totals["folds"][0]
    L, I = rsa._lib.lib(), rsa._lib.LinkEstInputs
    import ctypes as C
    P = E.linkest_params()
    for kw in (dict(K=3), dict(reserved=1), dict(peer=None), dict(stats=None)):
        f = dict(peer=peer.ctypes.data, stats=stats.ctypes.data, fwd=None, K=1, reserved=0)
        f.update(kw)
        assert L.rm_linkest_fold_tables(2, C.byref(I(**f)), C.byref(P), t.entry.ctypes.data, t.node.ctypes.data, t.pub_peer.ctypes.data,
                                        t.pub_stats.ctypes.data, t.totals.ctypes.data) == INVALID, kw
    assert L.rm_linkest_fold_tables(2, None, C.byref(P), t.entry.ctypes.data, t.node.ctypes.data, t.pub_peer.ctypes.data, t.pub_stats.ctypes.data,
                                    None) == INVALID
    assert not t.totals["folds"][0] and (t.pub_peer == -1).all()


def test_host_rule_under_sanitizers(rsa, tmp_path):
    """tests/cpp/linkest_host_san_test.cpp with rm_api_linkest.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "linkest_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_linkest.cpp"), os.path.join(ROOT, "tests", "cpp", "linkest_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
