"""bench.py as the benchmark driver runs it: a plain run prints the headline and nothing else, `--full` adds the roofline and the
legs measured after the timed region, and `--dump-outputs DIR` writes what the last timed step computed -- checked here against
the CPU oracle on the same ticks, and from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config")


def _bench(args, timeout=600):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), p.stdout[:1000]
    return lines[0]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _oracle_nodes(O, W, n, idx):
    nodes = W.make_nodes(n, idx)
    nd = O.NodeTable(n)
    nd.x, nd.y, nd.z = nodes.x, nodes.y, nodes.z
    return nd


def _check_tick(out, off, b, want):
    c = int(out["heard_per_tick"][b])
    assert c == want.count
    np.testing.assert_array_equal(out["pkt"][off:off + c], want.pkt)
    np.testing.assert_array_equal(out["dst"][off:off + c], want.dst)
    np.testing.assert_array_equal(out["verdict"][off:off + c], want.verdict)
    np.testing.assert_array_equal(out["rssi"][off:off + c], want.rssi)
    return off + c


def test_plain_run_prints_the_headline_and_dumps_the_last_step(O, tmp_path):
    """c2, 16 ticks per step, 1 warm-up + 3 timed steps: the timed ticks are 16 .. 63 of the source pool, the last step 48 .. 63;
    every one of its ticks is in the dump (10k nodes, 100 frames per tick: far below the budget) and equals the oracle's"""
    from radio_sim_amd import workload as W
    line = _bench(["--workload", "c2", "--steps", "3", "--warmup", "1", "--batch", "16", "--dump-outputs", str(tmp_path)])
    assert len(line) < 4096
    r = json.loads(line)
    assert all(k in r for k in HEADLINE), sorted(r)
    assert r["steps"] == 3 and r["warmup"] == 1 and r["value"] > 0 and r["ms_per_step"] > 0 and r["unit"] == "links/s"
    assert not {"roofline", "sequential_ticks", "with_host_transfer", "cpu_baseline"} & set(r)
    out = _load(str(tmp_path))
    assert {"heard_per_tick", "sampled_ticks", "pkt", "dst", "verdict", "rssi"} <= set(out)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    np.testing.assert_array_equal(out["sampled_ticks"], np.arange(16))
    assert out["heard_per_tick"][-1] == r["config"]["heard_links_last_tick"] > 0
    nd = _oracle_nodes(O, W, 10_000, 2)
    mdl = O.model(O.MODEL_LOGDIST)
    off = 0
    for b in range(16):
        src = W.choose_sources(10_000, 100, 0xC0FFEE02, 48 + b)
        off = _check_tick(out, off, b, O.tick(mdl, nd, nd.packets(src, 0, W.AIR_US)))
    assert off == len(out["dst"])


def test_default_workload_dump_is_a_fixed_sample_within_64_mb(O, tmp_path):
    """the flagship shape (c3: 128 ticks of 1000 frames over 100k nodes per step) holds more links than the budget: a seeded
    sample of whole ticks, the same in two runs with the same arguments, two of its ticks equal to the oracle's"""
    from radio_sim_amd import workload as W
    runs = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        r = json.loads(_bench(["--steps", "1", "--warmup", "0", "--dump-outputs", d]))
        assert r["steps"] == 1 and r["config"]["ticks_per_step"] == 128
        runs.append(_load(d))
    out, again = runs
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    for k in out:
        np.testing.assert_array_equal(out[k], again[k])
    picked = [int(b) for b in out["sampled_ticks"]]
    assert len(out["heard_per_tick"]) == 128 and 0 < len(picked) < 128 and "sampled_links" not in out
    nd = _oracle_nodes(O, W, 100_000, 3)
    mdl = O.model(O.MODEL_LOGDIST, ld_sigma_db=4.0, ld_seed=0xC0FFEE)
    starts = np.concatenate([[0], np.cumsum(out["heard_per_tick"][picked]).astype(np.int64)])
    for j in (0, len(picked) - 1):
        b = picked[j]
        src = W.choose_sources(100_000, 1000, 0xC0FFEE03, b)       # one step, no warm-up: the last step is ticks 0 .. 127
        _check_tick(out, int(starts[j]), b, O.tick_mt(mdl, nd, nd.packets(src, 0, W.AIR_US), cap=1 << 20))


def test_full_run_keeps_the_extra_keys():
    r = json.loads(_bench(["--workload", "c2", "--steps", "3", "--warmup", "1", "--batch", "16", "--no-host-transfer", "--full"]))
    assert all(k in r for k in HEADLINE)
    assert "roofline" in r and "sequential_ticks" in r and "cpu_baseline" in r and r["roofline"]["kernel"]
