"""The C++ mirror's clear-channel assessment (LogDistanceRadioMedium::getChannelEnergy / isChannelClear,
radio-sim_amd/host/radiomedium.hpp) against the Python engine: the same packets through rm_transmit, the same bits."""
import os
import subprocess

import numpy as np
import pytest

from util import KINDS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "energy_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "energy_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def test_mirror_energy_equals_the_engine(tmp_path, rsa, O):
    from radio_sim_amd import workload as W
    n, sigma, seed, t, thr = 2000, 4.0, 77, 600, -88.0
    src = W.make_nodes(n, 2)
    rng = np.random.default_rng(9)
    senders = rng.choice(n, 30, replace=False)
    starts = rng.integers(0, 500, 30)
    starts.sort()
    ask = rng.choice(n, 20, replace=False)
    ask[0] = senders[0]
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(src.x, src.y)]
    lines += [str(len(senders))] + ["%d %d 254" % (s, st) for s, st in zip(senders, starts)]
    lines += ["%d %.17g %d" % (t, thr, len(ask))] + [str(j) for j in ask]
    path = os.path.join(str(tmp_path), "energy.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout
    got = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("energy")]
    assert [int(g[1]) for g in got] == ask.tolist()

    nd = O.NodeTable(n)
    nd.x, nd.y = src.x, src.y
    eng = rsa.Engine(0)
    try:
        eng.upload_table(nd)
        eng.set_model(KINDS["logdist"], ld_sigma_db=sigma, ld_seed=seed, flags=1)
        eng.seed(1)
        for s, st in zip(senders, starts):
            eng.transmit(int(s), start_us=int(st), hex_length=254)
        energy, flags = eng.channel_energy(t, nodes=ask, cca_threshold_dbm=thr)
    finally:
        eng.close()
    assert (energy > -100.0).sum() >= 10 and (flags & 2).any() and not (flags & 2).all() and flags[0] & 1
    assert [int(g[2], 16) for g in got] == energy.view(np.uint64).tolist()
    assert [int(g[3]) for g in got] == [0 if f & 2 else 1 for f in flags]
