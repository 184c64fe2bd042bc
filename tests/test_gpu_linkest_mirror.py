"""The C++ mirror with the link estimator (GpuRadioMedium::setLinkEstimator / foldLinkEstimator / getLinkEstimates,
radio-sim_amd/host/radiomedium.hpp) on UDGM cliques: a text scene in -- ticks, neighbour-table updates that fill the watch table
from empty, a changed watch row, a fold behind every step --; every node's entries, peers and data-step state and the totals
out, against tests/linkest_ref.py fed the reference's watch table (tests/nbtable_ref.py) over ticks the oracle evaluates."""
import os
import subprocess

import numpy as np
import pytest

import linkest_ref as R
import nbtable_ref as NB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "linkest_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "linkest_mirror_test")
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


class Logged(NB.Driver):
    """the neighbour tables' CPU driver with an estimator behind it; it keeps what the scene did, so that the mirror can be told
    to do the same"""

    def __init__(self, nd, K, p):
        super().__init__(nd, "udgm", NB.UDGM, K, **NB.FILL)
        self.ops, self.est = [], R.Ref(nd.n, K, p)

    def tick(self, t_begin, t_end, src, start, air):
        self.ops.append("tick %d %s" % (t_begin, _list(src)))
        return super().tick(t_begin, t_end, src, start, air)

    def update(self, res, time_us, pin=None, slot=0):
        self.ops.append("update %d 0" % time_us)
        super().update(res, time_us, pin, slot)

    def watch(self, nodes, rows):
        for j, row in zip(nodes, rows):
            self.ops.append("watch %d %s" % (j, _list(row)))
        super().watch(nodes, rows)

    def fold(self):
        self.ops.append("fold 0")
        self.est.fold(self.ref.tab.peer.copy(), self.ref.tab.t.astype(R.LINK_STATS), None)


def _expected(d):
    est, K = d.est, d.K
    lines = ["refused 1", "on %d" % K]
    for j in range(est.n):
        lines += ["est " + " ".join(str(int(v)) for v in est.entry[j, k]) for k in range(K)]
        lines.append("peers " + " ".join(str(int(est.entry[j, k]["peer"])) for k in range(K)))
        lines.append("state " + " ".join(str(int(v)) for v in est.node[j]))
    tot = est.totals()
    lines.append("totals " + " ".join(str(tot[f]) for f in R.TOTALS))
    return lines + ["tables 1", "off 1"]


@pytest.mark.parametrize("n,K,p", [(64, 4, R.params(beacon_window=2)), (65, 1, R.params(beacon_window=1, beacon_alpha_q8=0)), (9, 8, R.params())])
def test_mirror_with_the_link_estimator(rsa, O, tmp_path, n, K, p):
    nd = NB.clique_nodes(n)
    d = Logged(nd, K, p)
    t = 0
    for b, lst in enumerate(NB.stride_lists(n, 12, 4)):
        d.update(d.tick(t, t + NB.TICK, lst, t + 100, NB.AIR), t + NB.TICK)
        t += NB.TICK
        if b == 7:        # (a changed row: node 0 drops what it watches, node 1 watches node 0 alone)
            d.watch([0, 1], np.array([[-1] * K, [0] + [-1] * (K - 1)], dtype=np.int32))
        d.fold()
    tot = d.est.totals()
    assert tot["folds"] == 12 and tot["beacon_samples"] >= n and tot["restarted"] >= n and tot["cleared"] >= 1 and tot["estimates"] >= n // 2
    lines = ["%d %d %d %d %d" % tuple(p[f] for f in ("beacon_window", "data_window", "beacon_alpha_q8", "data_alpha_q8", "max_etx")), str(K), str(n)]
    lines += ["%.17g %.17g" % (nd.x[i], nd.y[i]) for i in range(n)]
    lines += ["%d %d %d %d" % (NB.TICK, 100, NB.AIR // 32, len(d.ops))] + d.ops
    path = os.path.join(str(tmp_path), "linkest.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    assert out.stdout.splitlines() == _expected(d)
