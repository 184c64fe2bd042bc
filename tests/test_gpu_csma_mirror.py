"""The C++ mirror's CSMA-CA calls (LogDistanceRadioMedium::csmaSchedule / transmitCsmaBatch, radio-sim_amd/host/radiomedium.hpp) against
the oracle's chain (tests/csma_ref.py): n_exp, the outcome per packet, and the calls the medium makes -- generateTransmissionEvents per
sent packet in the order of its tick's expanded list, generateReceptionEvents per heard receiver in node order with the oracle's rssi
bits and verdict.  Two batches: the second begins with the first one's kept frames in the window."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import csma_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "csma_batch_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "csma_batch_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


class _Scene:
    """what csma_ref.Run asks of a scene: the mirror's tick begins at its sample, as transmitIfClear's"""

    def __init__(self, O, nd, sigma, seed, thr, times):
        self.nd, self.threshold, self._times = nd, thr, times
        self.params = dict(ld_sigma_db=sigma, ld_seed=seed, ld_flags=1)

    def model(self, O):
        return O.model(O.MODEL_LOGDIST, **self.params)

    def times(self, k):
        cca, start = self._times[k]
        return cca, cca, start


def test_mirror_csma_batch(tmp_path, O):
    # frames of 32 * 64 = 2048 us over ticks of 1000 us: a frame is on the air at the next two ticks' samples and gone at the third, so
    # that a deferred sender's retry can find the channel clear within a batch of three or four ticks
    n, sigma, seed, thr, hexlen = 3000, 4.0, 77, -88.0, 64
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    ticks = []
    for k in range(7):
        senders = rng.choice(n, 120, replace=False).astype(np.int32)
        if k == 2:
            senders[[5, 50]] = -1                                     # null senders: padding
        ticks.append((1000 * k - 72 if k else 0, 1000 * k, senders))
    p = SR.Params(3, 0, 2, 5)
    batches = [ticks[:4], ticks[4:]]
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)] + [str(len(batches))]
    for batch in batches:
        lines.append("%d %.17g %d %d %d %d %d" % (hexlen, thr, p.max_backoffs, p.min_be, p.max_be, p.seed, len(batch)))
        for cca, start, senders in batch:
            lines += ["%d %d %d %d" % (cca, start, cca, len(senders))] + [str(j) for j in senders]
    path = os.path.join(str(tmp_path), "csma_batch.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()
    assert got[-2:] == ["refused 1 1", "refused 1 1"]

    sc = _Scene(O, nd, sigma, seed, thr, [(cca, start) for cca, start, _ in ticks])
    chain = CR.Chain(O, nd, sc.model(O))
    air = 32 * hexlen
    want, retried, sent_late, most = [], 0, 0, 0
    first = 0
    for r, batch in enumerate(batches):
        run = SR.Run(O, sc, [s for _, _, s in batch], p, air=air, chain=chain, first_tick=first)
        first += len(batch)
        want.append("n_exp %d %s" % (r, " ".join(str(v) for v in run.n_exp)))
        want += ["pkt %d %d %d %d %d %d" % (r, run.status[o], run.attempts[o], run.tick[o], run.pkt[o], run.flags[o]) for o in range(len(run.status))]
        retried += int((run.attempts > 1).sum())
        sent_late += int(((run.status == SR.SENT) & (run.attempts > 1)).sum())
        for b in range(len(batch)):
            exp = run.exp[b]
            most = max(most, exp.count)
            for q, slot in enumerate(exp.slots):
                want.append("tx %d" % run.kept[b][slot])
                for k in range(*np.searchsorted(exp.raw.pkt, [q, q + 1])):
                    want.append("rx %d %d %016x %d" % (run.kept[b][slot], exp.raw.dst[k], np.float64(exp.raw.rssi[k]).view(np.uint64),
                                                       1 if exp.raw.verdict[k] == O.DELIVERED else 0))
    # (senders that retried, some of them sent by a retry, and a tick whose heard links outgrow the mirror's first buffer)
    assert retried > 40 and sent_late > 10 and most > 1024 and len(want) > 2000
    assert got[:-2] == want
