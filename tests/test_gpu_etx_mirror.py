"""The C++ mirror with the measured-route query (GpuRadioMedium::measuredRoutes, radio-sim_amd/host/radiomedium.hpp) against
tests/etx_ref.py: a text scene in, the medium's watched entries and its trees out.  The watched field's trees are the reference's
over the entries the medium itself reports; the (300, 4) band goes in as a caller's table."""
import os
import subprocess

import numpy as np
import pytest

import etx_ref as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "etx_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "etx_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _lines(run, t):
    tot = t["totals"]
    out = ["totals %d %d %d %d %d %d %d" % (run, tot["reached"], tot["roots"], tot["kept"], tot["switched"], tot["lost"], tot["max_cost"])]
    return out + ["row %d %d %d %d %d %d %d" % (run, j, t["cost"][j], t["parent"][j], t["slot"][j], t["link_cost"][j], t["children"][j])
                  for j in range(len(t["cost"]))]


def test_mirror_with_the_measured_route_query(rsa, tmp_path):
    n, K, sigma, seed, ticks, n_src = 300, 8, 4.0, 21, 100, 30
    rng = np.random.default_rng(6)
    side = float(np.sqrt(n * 2400.0))
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    roots = [0, 7, 0]
    band = E.band(300, 4)
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (a, b) for a, b in zip(x, y)]
    lines += ["%d 3000 64 %d" % (K, ticks)]
    for _ in range(ticks):
        src = np.sort(rng.choice(n, n_src, replace=False))
        lines.append("%d %s" % (n_src, " ".join(str(int(s)) for s in src)))
    lines += ["%d %s" % (len(roots), " ".join(str(r) for r in roots)), "4"]
    lines += ["%d %d %d" % (p, h, d) for p, h, d in zip(band[0].reshape(-1), band[1].reshape(-1), band[2].reshape(-1))]
    path = os.path.join(str(tmp_path), "etx.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    entries = [[int(v) for v in ln.split()[1:]] for ln in got if ln.startswith("entry ")]
    peer = np.full((n, K), -1, dtype=np.int32)
    heard, delivered = np.zeros((n, K), dtype=np.uint64), np.zeros((n, K), dtype=np.uint64)
    for j, k, p, h, d in entries:
        peer[j, k], heard[j, k], delivered[j, k] = p, h, d
    assert len(entries) > 1000 and (heard >= 4).sum() > 500 and ((delivered > 0) & (delivered < heard)).sum() > 100
    t0 = E.tree(peer, heard, delivered, E.prm(), roots)
    t1 = E.tree(peer, heard, delivered, E.prm(mode=E.BOTH), roots, t0["parent"])
    t2 = E.tree(peer, heard, delivered, E.prm(hysteresis=0), roots, t1["parent"])
    assert t0["totals"]["reached"] > 100 and t0["totals"]["roots"] == 2 and (t0["link_cost"] > 128).sum() > 20
    assert t1["totals"]["kept"] > 0 and t2["totals"]["switched"] > 0
    t3 = E.tree(*band, E.prm(max_link_cost=2000), [0])
    t4 = E.tree(*band, E.prm(max_link_cost=2000, mode=E.BOTH), [0], t3["parent"])
    want = [ln for ln in got if ln.startswith("entry ")]
    for run, t in enumerate((t0, t1, t2, t3, t4)):
        want += _lines(run, t)
    want += ["refused 1"]
    assert got == want
