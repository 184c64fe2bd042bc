"""CPU tier of the unicast outcome query.  1. the REFERENCE (tests/unicast_ref.py over the oracle) is
held to the conditions that make the scenes of tests/test_gpu_unicast.py worth running: if a scene misses one, the scene changes,
not the condition.  2. the library's pure host function rm_unicast_from_result against that reference, bit for bit.  3. the same
function in a stand-alone program under the host sanitizers (tests/cpp/unicast_host_san_test.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import errmodel_ref as R
import stats_ref as S
import unicast_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1

_REF = {}


def ref(name):
    """the scenes' reference slots, computed once, shared and left unchanged"""
    if name not in _REF:
        kind, _, arg = name.partition(":")
        seed = R.SEED if arg.endswith("e10") else None
        if kind == "lone":
            nd, srcs, start, air = R.scene_lone()
            _REF[name] = U.sinr_slots(nd, [srcs], [start], air, seed)
        elif kind == "batch":
            nd, lists, starts, air = R.scene_batch(arg.startswith("overlap"))
            _REF[name] = U.sinr_slots(nd, lists, starts, air, seed)
        else:
            _REF[name] = [U.media_slot(getattr(S, "scene_" + kind)())]
    return _REF[name]


def status_counts(slots, host=False):
    return U.counts(U.flat([s.outcome(w) for s, w in zip(slots, U.wants(slots, host))])["status"])


def segments(slots):
    return np.concatenate([np.diff(s.pkt_offset.astype(np.int64)) for s in slots])


# ---- 1. conditions on the reference alone ------------------------------------------------------------------------------------

# NONE / NOT_SENT / UNHEARD / INTERFERED / DELIVERED as the pick rule gives them (recorded, not required: the requirement is below)
RECORDED = {"lone:plain": (3, 0, 17, 11, 29), "lone:e10": (3, 0, 17, 29, 11),
            "batch:self:plain": (12, 3, 82, 45, 149), "batch:self:e10": (12, 3, 82, 128, 66),
            "batch:overlap:plain": (12, 3, 82, 51, 143), "batch:overlap:e10": (12, 3, 82, 137, 57),
            "udgm": (13, 0, 87, 82, 118), "n2n": (3, 0, 17, 17, 23), "udgm_const": (9, 0, 57, 0, 134)}


@pytest.mark.parametrize("name", sorted(RECORDED) + ["null"])
def test_pick_rule_reaches_every_outcome(O, name):
    slots = ref(name)
    c = status_counts(slots)
    print(name, dict(zip(U.NAMES, c.tolist())))
    assert c[U.LOST] == 0
    if name == "null":   # six frames that every node hears: nothing interfered, nothing to miss but the source itself
        assert c[U.DELIVERED] >= 3 and c[U.UNHEARD] >= 1 and c[U.INTERFERED] == 0
        return
    assert c[U.UNHEARD] >= 8 and c[U.DELIVERED] >= 8 and c[U.NONE] >= 3
    if name != "udgm_const":   # (no interfered link in that medium's scene: waived for it and for null only)
        assert c[U.INTERFERED] >= 8
    assert c[U.NOT_SENT] == (3 if name.startswith("batch") else 0)   # the three padding entries
    assert tuple(c[:5]) == RECORDED[name]
    # a host list cannot carry the out-of-range values: they become "not asked"
    h = status_counts(slots, host=True)
    assert h[U.NONE] > c[U.NONE] and h[U.DELIVERED] == c[U.DELIVERED] and h[U.INTERFERED] == c[U.INTERFERED]


def test_segment_lengths(O):
    """segments longer than a wave where the medium has them (about six nodes are in the stochastic UDGM scene's range and a tenth of
    the matrix is set: their longest segments have 15 and 44 links), empty ones in the batches, single links in udgm"""
    for name in ("lone:plain", "batch:self:plain", "batch:overlap:plain", "udgm_const", "null"):
        assert segments(ref(name)).max() > 64, name
    for name in ("batch:self:plain", "batch:overlap:plain"):
        assert (segments(ref(name)) == 0).sum() == 3
        assert max(s.count for s in ref(name)) > 16384 and any(len(s.src) == 0 for s in ref(name))
    assert (segments(ref("udgm")) == 1).any()
    assert segments(ref("udgm")).max() == 15 and segments(ref("n2n")).max() == 44


def test_ack_round_trip_conditions(O):
    nd, srcs, _, _ = R.scene_lone()
    data, want, d_out, ack, a_want, a_out = U.ack_round_trip(nd, srcs, R.SEED)
    reply = d_out["reply_src"]
    sent = reply[reply >= 0]
    assert len(sent) == len(set(sent.tolist())) >= 8                     # the chosen destinations are distinct
    assert (reply[3::4] == -1).all() and (d_out["status"][3::4] == U.UNHEARD).all()   # holes by construction
    assert (a_out["status"] == U.DELIVERED).sum() >= 8                   # acknowledgements that arrive
    assert (a_out["status"][reply < 0] == U.NOT_SENT).all()
    print("data", U.counts(d_out["status"]).tolist(), "ack", U.counts(a_out["status"]).tolist())


def test_outcome_on_a_hand_made_tick():
    off = np.array([0, 0, 1, 4, 4, 7], dtype=np.uint32)
    dst = np.array([5, 2, 4, 8, 1, 3, 9])
    ver = np.array([2, 1, 2, 2, 2, 1, 2], dtype=np.uint8)
    rssi, sinr = -np.arange(7.0), np.arange(7.0)
    out = U.outcome(10, [0, 6, 7, -1, 0], off, dst, ver, rssi, sinr, [0, 5, 2, 4, 9, 3])
    np.testing.assert_array_equal(out["status"], [U.UNHEARD, U.DELIVERED, U.INTERFERED, U.NOT_SENT, U.DELIVERED, U.NONE])
    np.testing.assert_array_equal(out["link"], [-1, 0, 1, -1, 6, -1])
    np.testing.assert_array_equal(out["reply_src"], [-1, 5, -1, -1, 9, -1])
    assert np.isnan(out["rssi"][[0, 3, 5]]).all() and out["sinr"][4] == 6.0 and out["rssi"][2] == -1.0
    lost = U.outcome(10, [0, 6, 7, -1, 0], off, dst, ver, rssi, None, [0, 5, -1, 4, 9], lost=True)
    np.testing.assert_array_equal(lost["status"], [U.LOST, U.LOST, U.NONE, U.LOST, U.LOST])
    assert np.isnan(lost["sinr"]).all()


# ---- 2. rm_unicast_from_result against the reference ---------------------------------------------------------------------------

class _Result:
    """a slot packed the way a host result carries it (pkt_rssi: one rssi per packet, no per-link column)"""

    def __init__(self, s, sinr, pkt_rssi=None):
        self.count, self.pkt_offset, self.dst, self.verdict = s.count, s.pkt_offset, s.dst, s.verdict
        self.rssi = None if pkt_rssi is not None else s.rssi
        self.pkt_rssi = pkt_rssi
        self.sinr = s.sinr if sinr else None


def _from_result_cases():
    for name in ("lone:e10", "batch:overlap:e10", "batch:self:plain", "udgm", "udgm_const", "n2n", "null"):
        yield name


@pytest.mark.parametrize("name", list(_from_result_cases()))
def test_from_result_matches_the_reference(rsa, O, name):
    slots = ref(name)
    media = ":" not in name
    for s, want in zip(slots, U.wants(slots, host=True)):
        layouts = [("rssi", None)]
        if media:   # the reference's media: a link's rssi is its packet's transmit power (checked: the layouts must agree)
            power = getattr(S, "scene_" + name)()[3]["txpower"].astype(np.float64)
            np.testing.assert_array_equal(U.bits(np.repeat(power, np.diff(s.pkt_offset.astype(np.int64)))), U.bits(s.rssi))
            layouts.append(("pkt_rssi", power))
        for layout, power in layouts:
            for sinr in (False, True) if s.sinr is not None else (False,):
                exp = s.outcome(want, sinr=sinr)
                got = rsa.Engine.unicast_from_result(_Result(s, sinr, power), s.src, s.n_nodes, want)
                U.equal(got, exp, "%s %s sinr=%s" % (name, layout, sinr))
                for drop in U.FIELDS:   # every output pointer NULL in turn
                    keep = [f for f in U.FIELDS if f != drop]
                    part = rsa.Engine.unicast_from_result(_Result(s, sinr, power), s.src, s.n_nodes, want, fields=keep)
                    assert sorted(part) == sorted(keep)
                    U.equal(part, exp, "%s without %s" % (name, drop), fields=keep)
        if (s.src >= 0).all():   # without the sources every packet counts as sent
            U.equal(rsa.Engine.unicast_from_result(_Result(s, True), None, s.n_nodes, want), s.outcome(want), name + ": src NULL")


def test_from_result_refusals(rsa, O):
    import ctypes as C
    from radio_sim_amd import _lib
    s = ref("lone:plain")[0]
    want = s.want(host=True)
    for bad in (s.n_nodes, s.n_nodes + 5):
        w = want.copy()
        w[7] = bad
        with pytest.raises(rsa.RadioMediumError) as e:
            rsa.Engine.unicast_from_result(_Result(s, True), s.src, s.n_nodes, w)
        assert e.value.code == INVALID
    status = np.full(len(want), 0xEE, dtype=np.uint8)
    out = _lib.UnicastOut(status=status.ctypes.data)
    L = _lib.lib()
    assert L.rm_unicast_from_result(None, None, s.n_nodes, want.ctypes.data, C.byref(out)) == INVALID
    r = _lib.HostResult(count=0, n_packets=len(want))
    assert L.rm_unicast_from_result(C.byref(r), None, s.n_nodes, want.ctypes.data, None) == INVALID
    assert L.rm_unicast_from_result(C.byref(r), None, s.n_nodes, None, C.byref(out)) == INVALID
    assert (status == 0xEE).all()
    # a result without a link: every asked packet unheard
    assert L.rm_unicast_from_result(C.byref(r), None, s.n_nodes, want.ctypes.data, C.byref(out)) == 0
    np.testing.assert_array_equal(status, np.where(want >= 0, U.UNHEARD, U.NONE))


# ---- 3. the host function under the host sanitizers, in a stand-alone program ----------------------------------------------------

def test_host_function_under_sanitizers(rsa, tmp_path):
    """tests/cpp/unicast_host_san_test.cpp with rm_api_unicast.cpp compiled beside it under -fsanitize=address,undefined (host code
    only: the program has its own main and touches no device)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "unicast_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-x", "hip", os.path.join(csrc, "rm_api_unicast.cpp"), os.path.join(ROOT, "tests", "cpp", "unicast_host_san_test.cpp"),
                           "-L" + csrc, "-lradiomedium_hip", "-Wl,-rpath," + csrc, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
