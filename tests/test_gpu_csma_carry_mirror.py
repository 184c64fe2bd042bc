"""The C++ mirror's CSMA-CA batch with a carry (LogDistanceRadioMedium::transmitCsmaBatch taking and returning a
std::vector<rm_csma_carry>, radio-sim_amd/host/radiomedium.hpp): two halves, the second fed the first one's carry-out, against the
oracle's run over all ticks as ONE batch (tests/csma_ref.py, tests/csma_carry_ref.py) -- the outcome per own and per carried packet,
and the calls the medium makes, which are those of the whole."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import csma_carry_ref as KR
import csma_ref as SR
from test_gpu_csma_mirror import _Scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "csma_carry_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "csma_carry_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def test_mirror_csma_carry(tmp_path, O):
    # the scene of test_gpu_csma_mirror.py (frames of 2048 us over ticks of 1000 us), eight ticks cut 4 + 4
    n, sigma, seed, thr, hexlen = 3000, 4.0, 77, -88.0, 64
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26
    ticks = []
    for k in range(8):
        senders = rng.choice(n, 120, replace=False).astype(np.int32)
        if k == 2:
            senders[[5, 50]] = -1
        ticks.append((1000 * k - 72 if k else 0, 1000 * k, senders))
    p = SR.Params(3, 0, 2, 5)
    batches = [ticks[:4], ticks[4:]]
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)] + [str(len(batches))]
    for batch in batches:
        lines.append("%d %.17g %d %d %d %d %d" % (hexlen, thr, p.max_backoffs, p.min_be, p.max_be, p.seed, len(batch)))
        for cca, start, senders in batch:
            lines += ["%d %d %d %d" % (cca, start, cca, len(senders))] + [str(j) for j in senders]
    path = os.path.join(str(tmp_path), "csma_carry.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()
    assert got[-1] == "refused 1 1"

    sc = _Scene(O, nd, sigma, seed, thr, [(cca, start) for cca, start, _ in ticks])
    run = SR.Run(O, sc, [s for _, _, s in ticks], p, air=32 * hexlen)
    t_cca = [cca for cca, _, _ in ticks]
    want, sent_carried = [], 0
    for r, (first, last) in enumerate(((0, 4), (4, 8))):
        carry, ids = KR.carry_at(run, first, t_cca)
        own, carried = KR.tables_of(run, first, last, ids, carry)
        want.append("carry %d %d" % (r, len(ids)))
        for tag, t in (("pkt", own), ("car", carried)):
            want += ["%s %d %d %d %d %d %d" % (tag, r, t["status"][o], t["attempts"][o], t["tick"][o], t["pkt"][o], t["flags"][o])
                     for o in range(len(t["status"]))]
        sent_carried += int((carried["status"] == SR.SENT).sum())
        for b in range(first, last):
            exp = run.exp[b]
            for q, slot in enumerate(exp.slots):
                want.append("tx %d" % run.kept[b][slot])
                for k in range(*np.searchsorted(exp.raw.pkt, [q, q + 1])):
                    want.append("rx %d %d %016x %d" % (run.kept[b][slot], exp.raw.dst[k], np.float64(exp.raw.rssi[k]).view(np.uint64),
                                                       1 if exp.raw.verdict[k] == O.DELIVERED else 0))
    want.append("carry 2 %d" % int((run.status == SR.PENDING).sum()))
    # (senders carried over the cut, some of them sent in the second half)
    assert len(KR.carry_at(run, 4, t_cca)[1]) > 20 and sent_carried > 5
    assert got[:-1] == want
