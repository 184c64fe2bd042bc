"""The C++ mirror with per-node traffic counters (GpuRadioMedium::setStatistics / resetStatistics / getStatistics,
radio-sim_amd/host/radiomedium.hpp) against the oracle plus tests/stats_ref.py: a text scene in, the tables out.  One per-packet
section (transmit(), frames that overlap each other) and one CSMA-CA batch section (transmitCsmaBatch) after a reset; the setting
survives a parameter change through apply()."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import csma_ref as SR
import errmodel_ref as R
import stats_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stats_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "stats_mirror_test")
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


def _lines(t):
    out = ["totals %d %d" % (t.counted, t.skipped)]
    for i in np.flatnonzero(np.any([t.t[c] != 0 for c in S.COLS], axis=0)):
        out.append("node %d " % i + " ".join(str(int(t.t[c][i])) for c in S.COLS))
    return out


def test_mirror_with_statistics(tmp_path, O):
    n, sigma, seed, thr = 3000, 4.0, 77, -88.0
    params = dict(ld_sigma_db=sigma, ld_seed=seed, ld_flags=1)
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
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)]
    lines += [str(len(pp))] + ["%d %d %d" % (s, t, hex_pp) for s, t in pp]
    lines.append("%d %.17g %d %d %d %d %d" % (hexlen, thr, p.max_backoffs, p.min_be, p.max_be, p.seed, len(ticks)))
    for cca, start, senders in ticks:
        lines += ["%d %d %d %d" % (cca, start, cca, len(senders))] + [str(j) for j in senders]
    path = os.path.join(str(tmp_path), "stats.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    want = ["enabled 1"]
    rep, t = R.Replay(nd, params=params), S.Table(n)
    for s, start in pp:
        res, _ = rep.tick(start, [s], start, 32 * hex_pp)
        t.add_result(nd.packets([s], start, 32 * hex_pp), res, verdict=res.plain)
    assert t.t["rx_heard"].sum() > 100 and (t.t["rx_heard"] > t.t["rx_delivered"]).any()
    want += _lines(t)
    s0 = pp[0][0]
    want.append("one %d " % s0 + " ".join(str(int(t.t[c][s0])) for c in S.COLS))
    want.append("batch")
    sc = _Scene(nd, params, thr, [(cca, start) for cca, start, _ in ticks])
    run = SR.Run(O, sc, [s for _, _, s in ticks], p, air=32 * hexlen)
    want += ["pkt %d %d %d %d %d" % (run.status[o], run.attempts[o], run.tick[o], run.pkt[o], run.flags[o]) for o in range(len(run.status))]
    t = S.Table(n)
    for b in range(len(ticks)):
        t.add_expected(run.exp[b], int(run.n_exp[b]))
    assert t.t["tx_frames"].sum() == (run.status == SR.SENT).sum() > 100 and (run.attempts > 1).sum() > 10
    want += _lines(t)
    want.append("refused 1")
    assert got == want
