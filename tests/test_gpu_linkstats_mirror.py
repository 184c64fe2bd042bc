"""The C++ mirror with watched-link statistics (GpuRadioMedium::setLinkWatch / watchLinks / getLinkStatistics,
radio-sim_amd/host/radiomedium.hpp) against the oracle plus tests/linkstats_ref.py: a text scene in, the medium's calls and its
entries out.  One tick-mode section (frames that start together) and one per-packet section (transmit(), frames that overlap each
other); the watch rows survive a parameter change through apply(), and the entries equal the ABI's read."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import errmodel_ref as R
import linkstats_ref as K
import listen_ref as LR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "linkstats_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "linkstats_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def _rx(src, res, k, verdict, O):
    return "rx %d %d %016x %d" % (src, res.dst[k], np.float64(res.rssi[k]).view(np.uint64), 1 if verdict[k] == O.DELIVERED else 0)


def test_mirror_with_watched_links(tmp_path, O):
    n, sigma, seed, k_slots = 3000, 4.0, 77, 4
    params = dict(ld_sigma_db=sigma, ld_seed=seed, ld_flags=1)
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    # the tick: 24 frames of 64 hex characters (2048 us) that start together at 0, evaluated when the step to 1000 is done
    hex_t = 64
    tick = [int(s) for s in rng.choice(n, 24, replace=False)]
    # per packet: 24 frames of 254 hex characters (8128 us), one every 3000 us from 100 000 us on: each sees the two before it; the
    # sources are those of the tick again, so that a watched link is heard a second time
    hex_pp = 254
    pp = [(int(s), 100_000 + 3000 * i) for i, s in enumerate(tick)]
    rep = R.Replay(nd, params=params)
    res_t, _ = rep.tick(0, tick, 0, 32 * hex_t)
    res_p = [rep.tick(t, [s], t, 32 * hex_pp)[0] for s, t in pp]
    pairs = [(LR.packets(nd, tick, 0, 32 * hex_t), res_t)] + [(LR.packets(nd, [s], t, 32 * hex_pp), w) for (s, t), w in zip(pp, res_p)]
    verdicts = [res_t.plain] + [w.plain for w in res_p]
    rows = K.rows_first_heard(n, k_slots, pairs)
    table, matched, unmatched = K.table_of(n, k_slots, rows, pairs, verdicts)
    h, d = table.t["heard"], table.t["delivered"]
    assert matched >= 1000 and (h >= 2).sum() >= 100 and ((d > 0) & (d < h)).sum() >= 10 and all((h[:, s] > 0).any() for s in range(k_slots))
    watched = np.flatnonzero((rows >= 0).any(axis=1))

    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)]
    lines += ["%d %d" % (k_slots, len(watched))]
    for j in watched:   # (a row's trailing empty slots are left to the mirror)
        last = int(np.flatnonzero(rows[j] >= 0)[-1]) + 1
        lines.append("%d %d %s" % (j, last, " ".join(str(int(p)) for p in rows[j][:last])))
    lines += ["1000 %d" % len(tick)] + ["%d 0 %d" % (s, hex_t) for s in tick]
    lines += [str(len(pp))] + ["%d %d %d" % (s, t, hex_pp) for s, t in pp]
    path = os.path.join(str(tmp_path), "linkstats.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()

    want = ["enabled %d" % k_slots, "tick"]
    for q, s in enumerate(tick):
        want.append("tx %d" % s)
        want += [_rx(s, res_t, i, res_t.plain, O) for i in range(*np.searchsorted(res_t.pkt, [q, q + 1]))]
    want.append("packets")
    for (s, t), w in zip(pp, res_p):
        want.append("tx %d" % s)
        want += [_rx(s, w, i, w.plain, O) for i in range(w.count)]
    for j, s in zip(*np.nonzero(h)):
        want.append("entry %d %d %s" % (j, s, " ".join(str(int(v)) for v in table.t[j, s].tolist())))
    want += ["totals %d 0" % (1 + len(pp)), "same 1"]
    assert got == want
