"""The C++ mirror with receiver listening schedules (GpuRadioMedium::setListenSchedule / clearListenSchedules / getListenMissed,
radio-sim_amd/host/radiomedium.hpp) against the oracle plus tests/listen_ref.py: a text scene in, the medium's calls out.  One
tick-mode section (frames that start together) and one per-packet section (transmit(), frames that overlap each other); the
schedules survive a parameter change through apply(), and the counts equal the ABI's read."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import errmodel_ref as R
import listen_ref as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "listen_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "listen_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _rx(src, res, k, verdict, O):
    return "rx %d %d %016x %d" % (src, res.dst[k], np.float64(res.rssi[k]).view(np.uint64), 1 if verdict[k] == O.DELIVERED else 0)


def test_mirror_with_listening_schedules(tmp_path, O):
    n, sigma, seed = 3000, 4.0, 77
    params = dict(ld_sigma_db=sigma, ld_seed=seed, ld_flags=1)
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    # the tick: 24 frames of 64 hex characters (2048 us) that start together at 0, evaluated when the step to 1000 is done
    hex_t = 64
    tick = [int(s) for s in rng.choice(n, 24, replace=False)]
    # per packet: 16 frames of 254 hex characters (8128 us), one every 3000 us from 100 000 us on: each sees the two before it
    hex_pp = 254
    pp = [(int(s), 100_000 + 3000 * k) for k, s in enumerate(rng.choice(n, 16, replace=False))]
    last = (int(pp[0][0]), 400_000)
    # the reference before E13, then the schedule over the receivers it reaches
    rep = R.Replay(nd, params=params)
    res_t, _ = rep.tick(0, tick, 0, 32 * hex_t)
    res_p = [rep.tick(t, [s], t, 32 * hex_pp)[0] for s, t in pp]
    res_l, _ = rep.tick(last[1], [last[0]], last[1], 32 * hex_pp)
    sched, edges = LR.schedule(n, LR.SCHED_SEED, LR.reached_receivers([(w, w.plain) for w in [res_t] + res_p]))
    assert len(edges) == len(LR.EDGES)
    set_order = np.flatnonzero(sched["period_us"] != 0)

    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)]
    lines += [str(len(set_order))] + ["%d %d %d %d" % ((i,) + tuple(int(v) for v in sched[i])) for i in set_order]
    lines += ["1000 %d" % len(tick)] + ["%d 0 %d" % (s, hex_t) for s in tick]
    lines += [str(len(pp))] + ["%d %d %d" % (s, t, hex_pp) for s, t in pp]
    lines.append("%d %d %d" % (last[0], last[1], hex_pp))
    path = os.path.join(str(tmp_path), "listen.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    want, missed, flipped, kept = ["enabled 1", "tick"], np.zeros(n, dtype=np.uint64), 0, 0
    after, m = LR.apply(LR.packets(nd, tick, 0, 32 * hex_t), res_t, sched, res_t.plain)
    missed += m
    flipped += int((after != res_t.plain).sum())
    for q, s in enumerate(tick):
        want.append("tx %d" % s)
        want += [_rx(s, res_t, k, after, O) for k in range(*np.searchsorted(res_t.pkt, [q, q + 1]))]
    assert flipped >= 50
    want.append("packets")
    for (s, t), w in zip(pp, res_p):
        after, m = LR.apply(LR.packets(nd, [s], t, 32 * hex_pp), w, sched, w.plain)
        missed += m
        flipped += int((after != w.plain).sum())
        kept += int((after == O.DELIVERED).sum())
        want.append("tx %d" % s)
        want += [_rx(s, w, k, after, O) for k in range(w.count)]
    assert flipped >= 150 and kept >= 100
    want += ["missed %d %d" % (i, missed[i]) for i in np.flatnonzero(missed)]
    want += ["same 1", "cleared 0", "tx %d" % last[0]]
    want += [_rx(last[0], res_l, k, res_l.plain, O) for k in range(res_l.count)]
    assert got == want
