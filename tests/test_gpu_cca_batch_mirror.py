"""The C++ mirror's listen-before-talk call across a batch of ticks (LogDistanceRadioMedium::transmitIfClearBatch,
radio-sim_amd/host/radiomedium.hpp) against the oracle's chain (tests/cca_ref.py::Chain.gated_tick, tick by tick): the flags per tick
and sender, and the calls the medium makes -- generateTransmissionEvents per kept packet, generateReceptionEvents per heard receiver in
node order with the oracle's rssi bits and verdict; a deferred packet and a padding slot generate nothing.  Two batches: the second
begins with the first one's kept frames in the window."""
import os
import subprocess

import numpy as np
import pytest

import cca_ref as CR
import energy_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cca_batch_mirror_test.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "cca_batch_mirror_test")
HDR = os.path.join(ROOT, "radio-sim_amd", "host", "radiomedium.hpp")


def _build():
    lib = os.path.join(ROOT, "radio-sim_amd", "csrc")
    if (not os.path.exists(BIN)) or os.path.getmtime(BIN) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", BIN, SRC, "-L" + lib, "-lradiomedium_hip",
                               "-Wl,-rpath," + lib])
    return BIN


def test_mirror_batch_transmits_only_the_clear_ones(tmp_path, O):
    n, sigma, seed, thr, hexlen = 3000, 4.0, 77, -88.0, 254
    nd, rng = CR.uniform_nodes(O, n, 5)
    nd.channel[:] = 26          # (a Transciever's default channel)
    ticks = []
    for k in range(6):          # (t_begin = sample time, start): the mirror's tick begins at the sample, as transmitIfClear's
        senders = rng.choice(n, 120, replace=False).astype(np.int32)
        if k == 2:
            senders[[5, 50]] = -1                                     # null senders: padding
        if k in (3, 5):
            senders[:6] = ticks[k - 2][2][10:16]                      # nodes of two ticks before, once more: transmitting if kept then
        ticks.append((1000 * k - 72 if k else 0, 1000 * k, senders))
    assert all(len(np.unique(s[s >= 0])) == (s >= 0).sum() for _, _, s in ticks)
    batches = [ticks[:4], ticks[4:]]
    lines = ["%.17g %d %d" % (sigma, seed, n)] + ["%.17g %.17g" % (x, y) for x, y in zip(nd.x, nd.y)] + [str(len(batches))]
    for batch in batches:
        lines.append("%d %.17g %d" % (hexlen, thr, len(batch)))
        for cca, start, senders in batch:
            lines += ["%d %d %d %d" % (cca, start, cca, len(senders))] + [str(j) for j in senders]
    path = os.path.join(str(tmp_path), "cca_batch.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([_build(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "error" not in out.stdout, out.stdout[:2000]
    got = out.stdout.splitlines()
    assert got[-2:] == ["refused 1 1", "refused 1 1"]

    chain = CR.Chain(O, nd, O.model(O.MODEL_LOGDIST, ld_sigma_db=sigma, ld_seed=seed, ld_flags=1))
    air = 32 * hexlen
    want, deferred, transmitting, most = [], 0, 0, 0
    for r, batch in enumerate(batches):
        calls = []
        for b, (cca, start, senders) in enumerate(batch):
            flags, _, exp = chain.gated_tick(cca, senders, start, air, cca, thr)
            want.append("flags %d %d %s" % (r, b, "".join(str(int(f)) for f in flags)))
            deferred += int((flags != 0).sum())
            transmitting += int(((flags & R.ED_TRANSMITTING) != 0).sum())
            most = max(most, exp.count)
            for q, slot in enumerate(exp.slots):
                calls.append("tx %d" % senders[slot])
                for k in range(*np.searchsorted(exp.raw.pkt, [q, q + 1])):
                    calls.append("rx %d %d %016x %d" % (senders[slot], exp.raw.dst[k], np.float64(exp.raw.rssi[k]).view(np.uint64),
                                                       1 if exp.raw.verdict[k] == O.DELIVERED else 0))
        want += calls
    # (deferred and kept candidates, a node on the air from its own batch, and a tick whose heard links outgrow the mirror's first buffer)
    assert 40 < deferred < 600 and transmitting >= 1 and most > 1024 and len(want) > 2000
    assert got[:-2] == want
