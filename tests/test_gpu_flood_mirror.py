"""The C++ mirror with dissemination floods (GpuRadioMedium::setFlooding / floodSeed / floodSources / floodAdvance /
getFloodStatistics / floodTree, radio-sim_amd/host/radiomedium.hpp) on the `line` and `clique` scenes of tests/flood_ref.py: a text
scene in; every step's source list, every node's row and tree entry and the totals out, against the reference over ticks the oracle
evaluates."""
import os
import subprocess

import pytest

import flood_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "flood_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "flood_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


class Logged(F.Driver):
    """the CPU tier's driver; it keeps what the scene did, so that the mirror can be told to do the same"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.asked, self.seeded, self.ticks = [], None, []

    def seed(self, nodes, time_us):
        assert self.seeded is None
        self.seeded = (list(nodes), time_us)
        super().seed(nodes, time_us)

    def sources(self, time_us, cap):
        lst, count = super().sources(time_us, cap)
        self.asked.append((cap, count, [j for j in lst if j >= 0]))
        return lst, count

    def tick(self, t_begin, t_end, src, start, air):
        self.ticks.append((t_begin, t_end - t_begin, start - t_begin, air))
        return super().tick(t_begin, t_end, src, start, air)


def _expected(d):
    lines = ["refused 1"]
    lines += ["sources %d %d%s" % (k, count, "".join(" %d" % j for j in lst)) for k, (_, count, lst) in enumerate(d.asked)]
    tbl = d.ref.table()
    for j in range(d.ref.n):
        lines.append("row " + " ".join(str(tbl[f][j]) for f in F.NODE_FIELDS))
        lines.append("tree %d %d" % (tbl["parent"][j], tbl["hop"][j]))
    tot = d.ref.totals()
    lines.append("totals " + " ".join(str(tot[f]) for f in F.TOTALS))
    return lines + ["off 1"]


SCENES = {"line40": lambda mk: F.scene_line(mk, 40), "clique65_k1": lambda mk: F.scene_clique(mk, 65, 1),
          "clique64_k0": lambda mk: F.scene_clique(mk, 64, 0)}


@pytest.mark.parametrize("name", list(SCENES))
def test_mirror_with_floods(rsa, O, tmp_path, name):
    d = SCENES[name](Logged)
    assert d.seeded and d.asked and len(d.asked) == len(d.ticks)
    _, tick, start_at, air = d.ticks[0]
    assert air % 32 == 0 and all(t[1:] == (tick, start_at, air) for t in d.ticks)
    p, nd = d.ref.p, d.nd
    cap = d.asked[0][0]
    lines = ["%d %d %d %d %d %d" % (p["imin_us"], p["doublings"], p["max_intervals"], p["redundancy"], p["max_hops"], p["seed"]), str(nd.n)]
    lines += ["%.17g %.17g" % (nd.x[i], nd.y[i]) for i in range(nd.n)]
    lines += ["%d %d" % (len(d.seeded[0]), d.seeded[1]), " ".join(str(int(v)) for v in d.seeded[0])]
    lines += ["%d %d %d %d %d" % (len(d.ticks), tick, start_at, air // 32, cap), " ".join(str(t[0]) for t in d.ticks)]
    path = os.path.join(str(tmp_path), "flood.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    assert out.stdout.splitlines() == _expected(d)
