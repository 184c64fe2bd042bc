"""The C++ mirror with the route query (LogDistanceRadioMedium::routes, radio-sim_amd/host/radiomedium.hpp) against the Python
engine and tests/routes_ref.py on one scene: a text scene in, rows out."""
import os
import subprocess

import pytest

import neighbors_ref as N
import routes_ref as R
from test_gpu_cca import _engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "routes_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "routes_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _lines(d, out, tot):
    lines = ["totals %d %d %d %d" % (d, tot["reached"], tot["roots"], tot["max_cost"])]
    rb = N.bits(out["rssi"]).tolist()
    return lines + ["row %d %d %d %d %016x %d %d" % (d, j, out["cost"][j], out["parent"][j], rb[j], out["link_cost"][j], out["children"][j])
                    for j in range(len(rb))]


def test_mirror_with_the_route_query(rsa, O, tmp_path):
    nd, params, found = R.scene("n300_shadow", "MARGINAL")
    roots = [0, N.special(nd)["S"], 0]
    min_rssi = -99.0
    lines = ["%.17g %d %.17g %.17g %d" % (params["ld_sigma_db"], params["ld_seed"], params["ld_sensitivity_dbm"], min_rssi, nd.n)]
    lines += ["%.17g %.17g %.17g %d %d %.17g" % (nd.x[i], nd.y[i], nd.txpower[i], nd.channel[i], nd.enabled[i], nd.rxprob[i]) for i in range(nd.n)]
    lines += [str(len(roots)), " ".join(str(j) for j in roots)]
    path = os.path.join(str(tmp_path), "routes.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    eng = _engine(rsa, nd, params)
    try:
        want = []
        for d in R.DIRS:
            for q in (R.SETS["NONE"][0], R.SETS["MARGINAL"][0], dict(R.SETS["MARGINAL"][0], min_rssi_dbm=min_rssi)):
                res, tot = eng.routes(rsa.Engine.routes_params(direction=d, **q), roots)
                R.same(res, tot, R.tree(nd.n, found[d], roots, q), "python engine, dir=%d %s" % (d, q))
                want += _lines(d, res, tot)
    finally:
        eng.close()
    want += ["refused 1"]
    assert got == want
