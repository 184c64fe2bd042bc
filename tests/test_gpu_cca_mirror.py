"""The C++ mirror's listen-before-talk call (LogDistanceRadioMedium::transmitIfClear, radio-sim_amd/host/radiomedium.hpp) against
the oracle's chain (tests/cca_ref.py): the flags per sender, and the calls the medium makes -- generateTransmissionEvents per
kept packet, generateReceptionEvents per heard receiver in node order with the oracle's rssi bits and verdict; a deferred packet
generates nothing."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cca_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "cca_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def test_mirror_transmits_only_the_clear_ones(tmp_path, O):
    n, sigma, seed, thr, hexlen = 3000, 4.0, 77, -88.0, 254
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    rounds = [(1000 * r, 1000 * r - 72 if r else 0, rng.choice(n, 120, replace=False).astype(np.int32)) for r in range(4)]
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)] + [str(len(rounds))]
    for start, cca, senders in rounds:
        lines += ["%d %d %d %.17g %d" % (start, hexlen, cca, thr, len(senders))] + [str(j) for j in senders]
    path = os.path.join(str(tmp_path), "cca.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()
    assert got[-1] == "refused 1 1"

    chain = CR.Chain(O, nd, O.model(O.MODEL_LOGDIST, ld_sigma_db=sigma, ld_seed=seed, ld_flags=1))
    air = 32 * hexlen
    want, deferred = [], 0
    for r, (start, cca, senders) in enumerate(rounds):
        flags, _, exp = chain.gated_tick(cca, senders, start, air, cca, thr)       # (the mirror's tick begins at the sample)
        want.append("flags %d %s" % (r, "".join(str(int(f)) for f in flags)))
        deferred += int((flags != 0).sum())
        for q, slot in enumerate(exp.slots):
            want.append("tx %d" % senders[slot])
            for k in range(*np.searchsorted(exp.raw.pkt, [q, q + 1])):
                want.append("rx %d %d %016x %d" % (senders[slot], exp.raw.dst[k], np.float64(exp.raw.rssi[k]).view(np.uint64),
                                                   1 if exp.raw.verdict[k] == O.DELIVERED else 0))
    assert 40 < deferred < 400 and len(want) > 2000
    assert got[:-1] == want
