"""The host model of tools/linkest_latency.py's yardstick (HostLinkEst: E23 with numpy) against the reference of
tests/linkest_ref.py over its scenes, after every fold: the yardstick the measurement is compared with computes what the rule says.
No GPU, no oracle."""
import importlib.util
import os

import numpy as np
import pytest

import linkest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("linkest_latency", os.path.join(ROOT, "tools", "linkest_latency.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("n, K, p", [(2, 1, R.params()), (9, 2, R.params(beacon_window=1, data_window=1, beacon_alpha_q8=0, data_alpha_q8=255, max_etx=65535)),
                                     (65, 4, R.params()), (257, 8, R.params()), (65, 8, R.params(beacon_window=0)),
                                     (33, 4, R.params(data_window=0, max_etx=128))])
def test_host_model_against_the_reference(n, K, p):
    T = _tool()
    assert (T.LINK_STATS, T.ENTRY, T.NODE, T.TOTALS) == (R.LINK_STATS, R.ENTRY, R.NODE, R.TOTALS)
    h, ref = T.HostLinkEst(n, K, **p), R.Ref(n, K, p)
    for f, (peer, stats, fwd) in enumerate(R.scene(n, K, seed=11)):
        fw = None if f % 4 == 3 else fwd
        before = ref.pub_stats.copy(), ref.pub_peer.copy()
        h.fold(peer, stats["heard"], stats["delivered"], None if fw is None else (fw["next"], fw["acked"], fw["failed"]))
        ref.fold(peer, stats, fw)
        R.same(ref, h.entries(), h.nodes(), h.pub_peer, h.pub_stats, h.totals(), "n %d K %d fold %d" % (n, K, f))
        assert h.changed == int(((ref.pub_stats["heard"] != before[0]["heard"]) | (ref.pub_peer != before[1])).sum())
    got = R.conditions(ref)
    if p == R.params():       # (a window of 1 is never partly full, a cap of 128 leaves nothing in between)
        assert all(got.values()), got
