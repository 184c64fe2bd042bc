"""The C++ mirror with traffic schedules (GpuRadioMedium::setTrafficSchedule / generateTraffic / clearTrafficSchedules,
radio-sim_amd/host/radiomedium.hpp) against tests/traffic_ref.py: a text scene in, the windows' nodes out.  The schedules survive a
parameter change through apply() and a node table of another size (the engine drops its table, the mirror sets it again)."""
import os
import subprocess

import numpy as np
import pytest

import traffic_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "traffic_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "traffic_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _want(table, seed, lo, hi, cap):
    rows, count, tot, _ = T.generate(table, seed, lo, hi, cap)
    lines = [" ".join(["window %d" % b] + [str(i) for i in l]) for b, l in enumerate(T.lists_of(rows, count))]
    return lines + ["totals %d %d %d" % (tot["packets"], tot["coalesced"], tot["truncated"])], count, tot


def test_mirror_with_traffic_schedules(tmp_path):
    n, more, seed, cap = 300, 45, 0xFEEDFACE12345678, 40
    rng = np.random.default_rng(15)
    xy = rng.uniform(0, 500, (n + more, 2))
    # every third node sends: period 700 .. 5000 us, jitter 0, 1, anything or the period; node 7 twice (the last call wins)
    sched = []
    for i in range(0, n, 3):
        p = int(rng.integers(700, 5000))
        sched.append((i, p, int(rng.integers(0, p)), (0, 1, int(rng.integers(0, p + 1)), p)[(i // 3) % 4]))
    sched.append((7, 900, 899, 900))
    sched.append((6, 100, 0, 0))
    sched.append((6, 0, 0, 0))          # ... and node 6 is switched off again
    table = [(0, 0, 0)] * n
    for i, p, ph, j in sched:
        table[i] = (p, ph, j)
    lo = [10000, 11000, 12000, 12000, 15000, 15800]
    hi = [11000, 12000, 12000, 13500, 15800, 15801]
    lines = ["%d %d %d" % (seed, cap, n)] + ["%.17g %.17g" % (x, y) for x, y in xy[:n]]
    lines += [str(len(sched))] + ["%d %d %d %d" % s for s in sched]
    lines += [str(len(lo))] + ["%d %d" % w for w in zip(lo, hi)]
    lines += [str(more)] + ["%.17g %.17g" % (x, y) for x, y in xy[n:]]
    path = os.path.join(str(tmp_path), "traffic.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    first, count, tot = _want(table, seed, lo, hi, cap)
    assert count.max() > cap and tot["truncated"] > 0 and tot["coalesced"] > 0 and count[2] == 0
    # the further nodes have no schedule: the same lists from the table the mirror set again
    again, _, _ = _want(table + [(0, 0, 0)] * more, seed, lo, hi, cap)
    assert again == first
    want = ["enabled 1", "generate"] + first + ["grown %d" % (n + more)] + again + ["bad 0", "cleared 0", "refused 1"]
    assert got == want
