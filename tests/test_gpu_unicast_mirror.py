"""The C++ mirror's unicast outcome query (GpuRadioMedium::unicastOutcomes and LogDistanceRadioMedium::unicastOutcomes over CSMA-CA
outcomes, radio-sim_amd/host/radiomedium.hpp; extension E12) against the oracle plus tests/unicast_ref.py: a text scene in, the
outcomes out.  A tick-mode step, a transmitIfClear() while the step's frames are still on the air, and a transmitCsmaBatch() are
each followed by the query; every printed status, link, rssi and sinr is compared exactly."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import csma_ref as SR
import unicast_ref as U
from test_gpu_stats_mirror import _Scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "unicast_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "unicast_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _lines(out):
    return ["%d %d %016x %016x" % (out["status"][k], out["link"][k], int(U.bits(out["rssi"])[k]), int(U.bits(out["sinr"])[k]))
            for k in range(len(out["status"]))]


def test_mirror_unicast_outcomes(tmp_path, O):
    n, sigma, seed, thr = 3000, 4.0, 77, -88.0
    params = dict(ld_sigma_db=sigma, ld_seed=seed, ld_flags=1)
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    chain = CR.Chain(O, nd, O.model(O.MODEL_LOGDIST, **params))
    # 1. the step: 40 frames of 254 hex characters (8128 us) that all start at 0
    hex1 = 254
    srcs = rng.choice(n, 40, replace=False).astype(np.int32)
    step = U.Slot(n, srcs, chain.plain_tick(0, srcs, 0, 32 * hex1))
    want1 = step.want(host=True)
    out1 = step.outcome(want1)
    # 2. listen before talk at 1000 us, the step's frames still on the air: some of the 150 candidates defer
    hex2, cca, start = 64, 1000, 1200
    cand = rng.choice(n, 150, replace=False).astype(np.int32)
    cand[[3, 70]] = -1
    flags, _, exp = chain.gated_tick(cca, cand, start, 32 * hex2, cca, thr)
    clear = U.Slot(n, np.where(flags != 0, -1, cand), exp)
    want2 = clear.want(host=True)
    out2 = clear.outcome(want2)
    assert (flags != 0).sum() >= 5 and (out2["status"] == U.NOT_SENT).sum() >= 5
    # 3. the CSMA-CA batch: four ticks well after everything has left the air (the scene of tests/test_gpu_stats_mirror.py)
    hex3, t0 = 64, 200_000
    ticks = []
    for k in range(4):
        senders = rng.choice(n, 120, replace=False).astype(np.int32)
        if k == 2:
            senders[[5, 50]] = -1
        ticks.append((t0 + 1000 * k - (72 if k else 0), t0 + 1000 * k, senders))
    p = SR.Params(3, 0, 2, 5)
    sc = _Scene(nd, params, thr, [(c, s) for c, s, _ in ticks])
    run = SR.Run(O, sc, [s for _, _, s in ticks], p, air=32 * hex3)
    slots = [U.Slot(n, run.kept[T], run.exp[T]) for T in range(len(ticks))]
    want_slots = U.wants(slots, host=True)
    outs = [s.outcome(w) for s, w in zip(slots, want_slots)]
    want3 = np.full(len(run.status), 5, dtype=np.int32)
    out3 = U.empty(len(run.status))
    for o in np.flatnonzero(run.status == SR.SENT):
        T, i = int(run.tick[o]), int(run.pkt[o])
        want3[o] = want_slots[T][i]
        for f in U.FIELDS:
            out3[f][o] = outs[T][f][i]
    for out in (out1, out2, out3):
        c = U.counts(out["status"])
        assert c[U.DELIVERED] >= 8 and c[U.UNHEARD] >= 5 and c[U.NONE] >= 1, c
    assert U.counts(out1["status"])[U.INTERFERED] + U.counts(out3["status"])[U.INTERFERED] >= 8

    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)]
    lines += ["%d %d" % (len(srcs), hex1)] + ["%d %d" % (s, w) for s, w in zip(srcs, want1)]
    lines += ["%d %.17g %d %d %d" % (hex2, thr, cca, start, len(cand))] + ["%d %d" % (s, w) for s, w in zip(cand, want2)]
    lines.append("%d %.17g %d %d %d %d %d" % (hex3, thr, p.max_backoffs, p.min_be, p.max_be, p.seed, len(ticks)))
    o = 0
    for c, s, senders in ticks:
        lines.append("%d %d %d %d" % (c, s, c, len(senders)))
        for j in senders:
            lines.append("%d %d" % (j, want3[o]))
            o += 1
    path = os.path.join(str(tmp_path), "unicast.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    res = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert "error" not in res.stdout, res.stdout[:2000]
    got = res.stdout.splitlines()

    exp_lines = ["refused 1", "step"] + _lines(out1)
    exp_lines += ["clear", "flags " + " ".join(str(int(f)) for f in flags)] + _lines(out2)
    exp_lines += ["csma"] + ["pkt %d %d %d" % (run.status[k], run.tick[k], run.pkt[k]) for k in range(len(run.status))] + _lines(out3)
    assert got == exp_lines
