"""The C++ mirror with the neighbour query (LogDistanceRadioMedium::neighbors / watchStrongest, radio-sim_amd/host/radiomedium.hpp)
against the Python engine and tests/neighbors_ref.py on one scene: a text scene in, rows out.  watchStrongest's rows are the
RM_NB_HEARS rows and survive a node table of another size."""
import os
import subprocess

import numpy as np
import pytest

import neighbors_ref as N
from test_gpu_cca import _engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "neighbors_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "neighbors_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _lines(tag, d, nodes, out):
    lines = []
    for e, j in enumerate(nodes):
        links = ["%d:%016x" % (p, b) for p, b in zip(out["peer"][e].tolist(), N.bits(out["rssi"][e]).tolist()) if p >= 0]
        lines.append(" ".join(["%s %d %d %d" % (tag, d, j, out["degree"][e])] + links))
    return lines


def test_mirror_with_the_neighbour_query(rsa, O, tmp_path):
    nd, params, found = N.scene("n300_shadow")
    K, WK = 6, 4
    listed = [int(j) for j in np.random.default_rng(3).permutation(nd.n)[:25]]
    lines = ["%.17g %d %d %d %d" % (params["ld_sigma_db"], params["ld_seed"], K, WK, nd.n)]
    lines += ["%.17g %.17g %.17g %d %d %.17g" % (nd.x[i], nd.y[i], nd.txpower[i], nd.channel[i], nd.enabled[i], nd.rxprob[i]) for i in range(nd.n)]
    lines += [str(len(listed)), " ".join(str(j) for j in listed)]
    path = os.path.join(str(tmp_path), "neighbors.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    eng = _engine(rsa, nd, params)
    try:
        want = []
        for d in (N.HEARD_BY, N.HEARS):
            full, part = eng.neighbors(d, K), eng.neighbors(d, K, nodes=listed)
            N.same(full, N.rows(nd, params, d, K, None, found[d]), "python engine, dir=%d" % d)
            want += _lines("row", d, range(nd.n), full) + _lines("list", d, listed, part)
        hears = eng.neighbors(N.HEARS, WK)["peer"]
    finally:
        eng.close()
    want += ["refused 1", "watch 1 %d" % WK]
    want += [" ".join(["peers %d" % i] + [str(p) for p in hears[i].tolist()]) for i in range(nd.n)]
    want += ["kept 1"]
    assert got == want
