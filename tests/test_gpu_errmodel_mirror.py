"""The C++ mirror with a frame error model (LogDistanceRadioMedium::setErrorModel / getErrorModel, radio-sim_amd/host/radiomedium.hpp)
against the oracle plus tests/errmodel_ref.py: a text scene in, the medium's calls out -- generateTransmissionEvents per packet,
generateReceptionEvents per heard receiver in node order with the oracle's rssi bits and the verdict after E10.  One per-packet section
(transmit(), frames that overlap each other) and one CSMA-CA batch section (transmitCsmaBatch, tests/csma_ref.py's chain)."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import csma_ref as SR
import errmodel_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "errmodel_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "errmodel_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


class _Scene:
    def __init__(self, nd, params, thr, times):
        self.nd, self.params, self.threshold, self._times = nd, params, thr, times

    def model(self, O):
        return O.model(O.MODEL_LOGDIST, **self.params)

    def times(self, k):
        cca, start = self._times[k]
        return cca, cca, start


def _rx(src, res, k, verdict, O):
    return "rx %d %d %016x %d" % (src, res.dst[k], np.float64(res.rssi[k]).view(np.uint64), 1 if verdict[k] == O.DELIVERED else 0)


def test_mirror_with_the_error_model(tmp_path, O):
    n, sigma, seed, thr, em_seed = 3000, 4.0, 77, -88.0, R.SEED
    params = dict(ld_sigma_db=sigma, ld_seed=seed, ld_flags=1, ld_sensitivity_dbm=-103.0, ld_noise_dbm=-100.0, ld_capture_db=R.NINF)
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    # per packet: 16 frames of 254 hex characters (8128 us), one every 3000 us: each sees the two before it on the air
    hex_pp = 254
    pp = [(int(s), 3000 * k) for k, s in enumerate(rng.choice(n, 16, replace=False))]
    # the batch: four ticks well after the last of them has left the air, frames of 2048 us over ticks of 1000 us
    hexlen, t0 = 64, 200_000
    ticks = []
    for k in range(4):
        senders = rng.choice(n, 120, replace=False).astype(np.int32)
        if k == 2:
            senders[[5, 50]] = -1
        ticks.append((t0 + 1000 * k - (72 if k else 0), t0 + 1000 * k, senders))
    p = SR.Params(3, 0, 2, 5)
    lines = ["%.17g %d %d -103 -100 %d" % (sigma, seed, n, em_seed)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)]
    lines += [str(len(pp))] + ["%d %d %d" % (s, t, hex_pp) for s, t in pp]
    lines.append("%d %.17g %d %d %d %d %d" % (hexlen, thr, p.max_backoffs, p.min_be, p.max_be, p.seed, len(ticks)))
    for cca, start, senders in ticks:
        lines += ["%d %d %d %d" % (cca, start, cca, len(senders))] + [str(j) for j in senders]
    path = os.path.join(str(tmp_path), "errmodel.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    want = ["model 1 4 %d" % em_seed]
    rep = R.Replay(nd, params=params, seed=em_seed)
    flipped = kept = 0
    for s, t in pp:
        res, _ = rep.tick(t, [s], t, 32 * hex_pp)
        want.append("tx %d" % s)
        want += [_rx(s, res, k, res.verdict, O) for k in range(res.count)]
        flipped += int((res.verdict != res.plain).sum())
        kept += int((res.verdict == O.DELIVERED).sum())
    assert flipped >= 50 and kept >= 50
    want.append("batch")
    sc = _Scene(nd, params, thr, [(cca, start) for cca, start, _ in ticks])
    run = SR.Run(O, sc, [s for _, _, s in ticks], p, air=32 * hexlen)
    want += ["pkt %d %d %d %d %d" % (run.status[o], run.attempts[o], run.tick[o], run.pkt[o], run.flags[o]) for o in range(len(run.status))]
    flipped = 0
    for b in range(len(ticks)):
        exp = run.exp[b]
        if exp.raw is None:
            continue
        v = R.apply_full(exp.new, exp.raw, em_seed)[0]
        flipped += int((v != exp.raw.verdict).sum())
        for q, slot in enumerate(exp.slots):
            want.append("tx %d" % run.kept[b][slot])
            want += [_rx(run.kept[b][slot], exp.raw, k, v, O) for k in range(*np.searchsorted(exp.raw.pkt, [q, q + 1]))]
    assert flipped >= 50 and (run.attempts > 1).sum() > 10
    want.append("refused 1")
    assert got == want
