"""The measured-route query without a GPU: the conditions the scenes of tests/etx_ref.py are meant to
have, asserted from the reference alone; and the pure host functions rm_etx_link_cost, rm_etx_combine and rm_etx_from_tables
against that reference.  Every comparison is exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import etx_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
CASES = E.cases()


def _p(rsa, p):
    return rsa.Engine.etx_params(**p)


def _follow_lowers_cost(t):
    par, cost = t["parent"], t["cost"]
    has = par >= 0
    return bool((cost[par[has]] < cost[has]).all())


# ---- 1. the scenes have what they are for ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, K", E.BANDS[:2])
@pytest.mark.parametrize("mode", E.MODES)
def test_band_conditions(n, K, mode):
    t = E.band(n, K)
    cur = E.tree(*E.band(n, K, seed=22), E.prm(mode=mode, **E.BAND_P), [0])["parent"]
    p = E.prm(mode=mode, hysteresis=0, **E.BAND_P)
    want = E.tree(*t, p, [0])
    assert want["totals"]["reached"] == n and want["totals"]["roots"] == 1
    cost, rounds, lowered = E.pull(*t, p, [0])
    np.testing.assert_array_equal(cost, want["cost"])                   # Dijkstra and synchronous pulling agree
    assert (lowered > 1).sum() > n // 2 and rounds > 10                 # most nodes are lowered more than once when pulled
    lc = np.array(E.link_costs(*t, p))
    far = np.where(lc > 0, t[0], 0)
    ties = ((lc > 0) & (want["cost"][far] + lc.astype(np.uint64) == want["cost"][:, None])).sum(axis=1)
    assert (ties[1:] >= 1).all() and (ties > 1).sum() >= 1              # some nodes choose among tied parents
    kept = []
    for h in (0, 64, 192, 1000):
        got = E.tree(*t, dict(p, hysteresis=h), [0], cur)
        np.testing.assert_array_equal(got["cost"], want["cost"])        # the cost stays the least cost
        assert _follow_lowers_cost(got)                                 # loop-free for every hysteresis
        tot = got["totals"]
        assert tot["kept"] + tot["switched"] == n - 1 and tot["lost"] == 0
        if h <= 192:
            assert tot["kept"] > 0 and tot["switched"] > 0
        kept.append(tot["kept"])
    assert kept[0] < kept[1] < kept[2] <= kept[3], kept


@pytest.mark.parametrize("n, K", E.BANDS[2:])
def test_chains(n, K):
    t = E.band(n, K)
    p = E.prm(**E.BAND_P)
    cost, rounds, lowered = E.pull(*t, p, [0])
    want = E.tree(*t, p, [0])
    np.testing.assert_array_equal(cost, want["cost"])
    assert rounds == n and want["totals"]["reached"] == n and want["parent"].tolist() == list(range(-1, n - 1))
    both = E.tree(*t, dict(p, mode=E.BOTH), [0])
    assert both["totals"]["reached"] == (1 if K == 1 else n)          # K = 1: no entry has its reverse


def test_keep_edge():
    s = E.keep_edge()
    t = E.tree(*s["tables"], s["prm"], s["roots"], s["cur"])
    assert t["cost"].tolist()[:10] == [0, 128, 128, 256, 128, 256, 256, 256, 256, 256] and (t["cost"][10:] == E.UNREACHED).all()
    assert (t["parent"][3], t["slot"][3], t["link_cost"][3]) == (4, 1, 320)      # exactly at cost + hysteresis: kept
    assert (t["parent"][5], t["slot"][5], t["link_cost"][5]) == (1, 0, 128)      # one unit above: switched
    assert (t["parent"][6], t["link_cost"][6]) == (1, 128)                       # cost[q] == cost[j]: never kept
    assert (t["parent"][7], t["slot"][7], t["link_cost"][7]) == (4, 2, 200)      # two slots: the cheaper, the lower of equals
    assert t["parent"][8] == 1 and (t["parent"][9], t["slot"][9]) == (1, 1)      # cur outside the table; (c, p, k): 1 before 4
    assert t["parent"][0] == -1 and t["parent"][10] == -1 and t["parent"][11] == -1
    assert t["totals"] == {"reached": 10, "roots": 1, "kept": 3, "switched": 2, "lost": 1, "max_cost": 256}
    assert t["children"].tolist() == [3, 4, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0]
    one_less = E.tree(*s["tables"], dict(s["prm"], hysteresis=191), s["roots"], s["cur"])
    assert one_less["parent"][3] == 1 and one_less["totals"]["kept"] == 2
    none = E.tree(*s["tables"], s["prm"], s["roots"])
    assert none["totals"]["kept"] == none["totals"]["switched"] == none["totals"]["lost"] == 0


def test_cost_edge():
    s = E.cost_edge()
    inb = E.tree(*s["tables"], s["prm"], s["roots"])
    reached = (inb["cost"] != E.UNREACHED).tolist()
    assert reached == [True, True, False, True, False, False, True, True, False, True, True, True, True, True, True, True, True, True, True]
    assert inb["cost"][[1, 3, 6, 7]].tolist() == [128, 128, 128, 2000] and inb["cost"][[10, 12, 14, 16, 18]].tolist() == [512, 512, 128, 128, 128]
    both = E.tree(*s["tables"], dict(s["prm"], mode=E.BOTH), s["roots"])
    assert (both["cost"][1:9] == E.UNREACHED).all()                   # the root's row holds none of them
    assert both["cost"][10] == 2000 and both["cost"][12] == E.UNREACHED and both["cost"][14] == E.UNREACHED
    assert both["cost"][16] == E.UNREACHED and both["cost"][18] == 256
    s0 = E.cost_edge_min0()
    t0 = E.tree(*s0["tables"], s0["prm"], s0["roots"])
    assert (t0["cost"] != E.UNREACHED).tolist() == [True, False, False, True]


def test_junk():
    s = E.junk()
    t = E.tree(*s["tables"], s["prm"], s["roots"], s["cur"])
    assert t["cost"].tolist() == [0, E.UNREACHED, 128, 288, 416, E.UNREACHED, E.UNREACHED, E.UNREACHED]
    assert (t["parent"][2], t["slot"][2]) == (0, 2) and (t["parent"][3], t["slot"][3]) == (2, 2)
    assert (t["parent"][4], t["slot"][4], t["link_cost"][4]) == (2, 3, 289)      # kept: 128 + 289 is within 416 + 64
    assert t["totals"] == {"reached": 4, "roots": 1, "kept": 2, "switched": 1, "lost": 4, "max_cost": 416}
    free = E.tree(*s["tables"], s["prm"], s["roots"])
    assert (free["parent"][4], free["slot"][4]) == (3, 2)


def test_root_lists():
    t = E.band(300, 4)
    p = E.prm(**E.BAND_P)
    lists = E.root_lists(300)
    assert [len(lists[k]) for k in ("list16384", "list16385", "list40000")] == [16384, 16385, 40000]
    assert E.tree(*t, p, lists["duplicates"])["totals"]["roots"] == 2
    assert E.tree(*t, p, lists["none"])["totals"] == {"reached": 0, "roots": 0, "kept": 0, "switched": 0, "lost": 0, "max_cost": 0}
    assert E.tree(*t, p, lists["all"])["totals"]["roots"] == 300
    assert E.tree(*t, p, lists["list40000"])["totals"]["roots"] == 20
    assert E.tree(*t, p, lists["outside"])["totals"]["roots"] == 3


def test_wide_is_shallow_and_wide():
    t = E.wide()
    for mode in E.MODES:
        w = E.tree_np(*t, E.prm(mode=mode, **E.BAND_P), [0, t[0].shape[0] - 1])
        assert w["totals"]["reached"] == t[0].shape[0] and w["totals"]["roots"] == 2 and w["totals"]["max_cost"] < 128 * 400


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_numpy_form_is_the_plain_form(name):
    s = dict(CASES)[name]
    for mode in E.MODES:
        p = dict(s["prm"], mode=mode)
        for cur in (None, s["cur"]) if s["cur"] is not None else (None,):
            a, b = E.tree(*s["tables"], p, s["roots"], cur), E.tree_np(*s["tables"], p, s["roots"], cur)
            E.same({f: b[f] for f in E.FIELDS}, b["totals"], a, "%s mode=%d" % (name, mode))


# ---- 2. the pure host functions -------------------------------------------------------------------------------------------------

def test_struct_layouts(rsa):
    import ctypes as C
    assert rsa.LINK_STATS_DTYPE == E.STATS_DTYPE
    assert C.sizeof(rsa.EtxParams) == 24 and C.sizeof(rsa.EtxTotals) == 32 and C.sizeof(rsa.EtxTables) == 24 and C.sizeof(rsa.EtxOut) == 40
    d = rsa.Engine.etx_params()
    assert (d.mode, d.reserved, d.min_heard, d.max_link_cost, d.hysteresis, d.reserved2) == (0, 0, 4, 2048, 192, 0)
    assert (rsa.ETX_INBOUND, rsa.ETX_BOTH) == (E.INBOUND, E.BOTH)


def test_link_cost_and_combine_against_the_reference(rsa):
    Hs = [0, 1, 3, 4, 5, 39, 40, 41, 127, 128, 1000, 2 ** 31, 2 ** 40 - 1, 2 ** 40, 2 ** 40 + 1, 2 ** 63, 2 ** 64 - 1]
    for mh, cap in ((4, 2000), (0, 128), (1, 65535), (2 ** 31, 65535), (40, 2048)):
        prm = rsa.Engine.etx_params(min_heard=mh, max_link_cost=cap)
        for H in Hs:
            Ds = {0, 1, 2, 3, H // 16, H // 15, H // 3, H // 2, max(H - 1, 0), H, H + 1, 2 * H, 2 ** 64 - 1}
            Ds |= {(128 * H) // cap, (128 * H) // cap + 1, max((128 * H) // cap - 1, 0)}
            for D in sorted(d for d in Ds if d < 2 ** 64):
                assert rsa.Engine.etx_link_cost(prm, H, D) == E.c_in(H, D, mh, cap), (mh, cap, H, D)
    cs = [0, 1, 127, 128, 129, 500, 501, 512, 2000, 2048, 65535, 65536, 2 ** 32 - 1]
    for a in cs:
        for b in cs:
            assert rsa.Engine.etx_combine(a, b) == E.combine(a, b)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_from_tables_against_the_reference(rsa, name):
    s = dict(CASES)[name]
    peer, heard, delivered = s["tables"]
    tables = (peer, E.stats(heard, delivered))
    for mode in E.MODES:
        p = dict(s["prm"], mode=mode)
        for cur in (None, s["cur"]) if s["cur"] is not None else (None,):
            want = E.tree(peer, heard, delivered, p, s["roots"], cur)
            got, tot = rsa.Engine.etx_from_tables(tables, _p(rsa, p), s["roots"], cur)
            assert set(got) == set(E.FIELDS)
            E.same(got, tot, want, "%s mode=%d cur=%s" % (name, mode, cur is not None))
        for f in E.FIELDS[1:]:
            got, tot = rsa.Engine.etx_from_tables(tables, _p(rsa, p), s["roots"], s["cur"], fields=(f,))
            assert set(got) == {"cost", f}
            E.same(got, tot, E.tree(peer, heard, delivered, p, s["roots"], s["cur"]), "%s mode=%d %s alone" % (name, mode, f))


def test_refusals_of_the_pure_functions(rsa):
    import ctypes as C
    L = rsa._lib.lib()
    peer, heard, delivered = E.band(4, 2)
    st = E.stats(heard, delivered)
    cost = np.zeros(4, dtype=np.uint64)
    out = rsa.EtxOut(cost=cost.ctypes.data)
    roots = np.array([0], dtype=np.int32)
    ok_t = rsa.EtxTables(peer=peer.ctypes.data, stats=st.ctypes.data, K=2, reserved=0)
    ok_p = rsa.Engine.etx_params()

    def call(n=4, t=ok_t, p=ok_p, r=roots.ctypes.data, nr=1, o=out):
        return L.rm_etx_from_tables(n, None if t is None else C.byref(t), None if p is None else C.byref(p), r, nr, None,
                                    None if o is None else C.byref(o), None)

    assert call() == 0
    assert call(o=None) == INVALID and call(o=rsa.EtxOut()) == INVALID and call(p=None) == INVALID and call(t=None) == INVALID
    assert call(n=-1, nr=0) == INVALID and call(nr=-1) == INVALID and call(r=None) == INVALID
    for kw in ({"K": 0}, {"K": 3}, {"K": 16}, {"reserved": 1}, {"peer": None}, {"stats": None}):
        t = rsa.EtxTables(**dict(dict(peer=peer.ctypes.data, stats=st.ctypes.data, K=2, reserved=0), **kw))
        assert call(t=t) == INVALID, kw
    for kw in ({"mode": 2}, {"mode": -1}, {"reserved": 1}, {"reserved2": 1}, {"min_heard": 2 ** 31 + 1}, {"max_link_cost": 127},
               {"max_link_cost": 65536}, {"hysteresis": 65536}):
        p = rsa.Engine.etx_params(**kw)
        assert rsa.Engine.etx_validate(p) == INVALID and call(p=p) == INVALID and rsa.Engine.etx_link_cost(p, 40, 40) is None, kw
    for kw in ({"min_heard": 2 ** 31}, {"min_heard": 0}, {"max_link_cost": 128}, {"max_link_cost": 65535}, {"hysteresis": 0}, {"hysteresis": 65535}, {"mode": 1}):
        assert rsa.Engine.etx_validate(rsa.Engine.etx_params(**kw)) == 0, kw
    for bad in ([4], [-1]):
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.etx_from_tables((peer, st), ok_p, bad)
        assert e.value.code == INVALID


def test_from_tables_under_sanitizers(rsa, tmp_path):
    """tests/cpp/etx_host_san_test.cpp with rm_api_etx.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "etx_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_etx.cpp"), os.path.join(ROOT, "tests", "cpp", "etx_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
