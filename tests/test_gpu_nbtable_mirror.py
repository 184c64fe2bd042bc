"""The C++ mirror with neighbour tables (GpuRadioMedium::setNeighbourTable / updateNeighbours / expireNeighbours /
getNeighbourTableStatistics, radio-sim_amd/host/radiomedium.hpp) on the UDGM scenes of tests/nbtable_ref.py: a text scene in; every
node's counters, peer row and entries and the totals out, against the reference over ticks the oracle evaluates."""
import os
import subprocess

import pytest

import nbtable_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "nbtable_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "nbtable_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _list(v):
    v = [] if v is None else [int(x) for x in v]
    return "%d%s" % (len(v), "".join(" %d" % x for x in v))


class Logged(R.Driver):
    """the CPU tier's driver; it keeps what the scene did, so that the mirror can be told to do the same"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.ops, self.shape = [], set()

    def tick(self, t_begin, t_end, src, start, air):
        self.shape.add((t_end - t_begin, start - t_begin, air))
        self.ops.append("tick %d %s" % (t_begin, _list(src)))
        return super().tick(t_begin, t_end, src, start, air)

    def update(self, res, time_us, pin=None, slot=0):
        self.ops.append("update %d %s" % (time_us, _list(pin)))
        super().update(res, time_us, pin, slot)

    def expire(self, time_us, pin=None):
        self.ops.append("expire %d %s" % (time_us, _list(pin)))
        super().expire(time_us, pin)

    def watch(self, nodes, rows):
        for j, row in zip(nodes, rows):
            self.ops.append("watch %d %s" % (j, _list(row)))
        super().watch(nodes, rows)


def _expected(d):
    lines = ["refused 1"]
    ref = d.ref
    for j in range(ref.n):
        lines.append("row " + " ".join(str(ref.cnt[f][j]) for f in R.NODE_FIELDS))
        lines.append("peers " + " ".join(str(-1 if ref.empty(j, k) else int(ref.tab.peer[j, k])) for k in range(ref.K)))
        lines += ["entry " + " ".join(str(int(v)) for v in ref.tab.t[j, k]) for k in range(ref.K)]
    tot = ref.totals()
    lines.append("totals " + " ".join(str(tot[f]) for f in R.TOTALS))
    return lines + ["off 1"]


SCENES = {"clique64_k4": lambda mk: R.scene_fill(mk, "clique", 64, 4), "clique65_k1": lambda mk: R.scene_fill(mk, "clique", 65, 1),
          "pins": R.scene_pins, "tie": R.scene_tie, "dup": R.scene_dup}


@pytest.mark.parametrize("name", list(SCENES))
def test_mirror_with_neighbour_tables(rsa, O, tmp_path, name):
    d = SCENES[name](Logged)
    assert d.kind == "udgm" and d.params == R.UDGM and d.steps >= 1 and len(d.shape) == 1
    tick, start_at, air = next(iter(d.shape))
    assert air % 32 == 0
    p, nd = d.ref.p, d.nd
    lines = ["%.17g %d %d %d %d" % (p["admit_rssi_dbm"], p["timeout_us"], p["min_heard"], p["evict_cost"], p["require_delivered"]), str(d.K), str(nd.n)]
    lines += ["%.17g %.17g" % (nd.x[i], nd.y[i]) for i in range(nd.n)]
    lines += ["%d %d %d %d" % (tick, start_at, air // 32, len(d.ops))] + d.ops
    path = os.path.join(str(tmp_path), "nbtable.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    assert out.stdout.splitlines() == _expected(d)
