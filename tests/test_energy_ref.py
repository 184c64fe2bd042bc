"""CPU tier of the channel energy query: the reference helper's Q80 restatement against the oracle, the
query's symbols at the boundary, and the reference scene's own conditions -- computed by the helper alone, so that a change
to the workload cannot hollow out tests/test_gpu_energy.py without this file noticing."""
import math
import os
import re

import numpy as np

import energy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_q80_restatement_agrees_with_the_oracle(O):
    L = O.lib()
    rng = np.random.default_rng(0xED)
    vals = [float(v) for v in 10.0 ** (rng.uniform(-140.0, 10.0, 20_000) / 10.0)]
    vals += [0.0, -1.0, 5e-324, 2.2250738585072009e-308, 2.0 ** -80, 2.0 ** -81, 2.0 ** -79,
             math.nextafter(2.0 ** -28, 0.0), 2.0 ** -28, math.nextafter(2.0 ** -28, 1.0), 2.0 ** -27, 1.0, 2.0 ** 46,
             2.0 ** 47, float("inf")]
    vals += [float(v) for v in 2.0 ** rng.uniform(-90.0, 50.0, 2_000)]
    bad = [v for v in vals if np.float64(R.from_fixed(R.to_fixed(v))).view(np.uint64) != np.float64(L.orc_fixed_roundtrip(v)).view(np.uint64)]
    assert len(vals) >= 20_000 and not bad, bad[:5]
    assert R.to_fixed(2.0 ** -80) == 1 and R.to_fixed(float("inf")) == R.Q80_MAX and R.to_fixed(5e-324) == 0


def test_query_symbols_at_the_boundary(rsa):
    from radio_sim_amd import _lib
    text = open(os.path.join(ROOT, "include", "radiomedium_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rm_channel_energy", "rm_channel_energy_device"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name)
    defs = dict(re.findall(r"#define\s+(RM_[A-Z_]+)\s+\(?(-?\d+)\)?", code))
    assert (defs["RM_CHANNEL_OWN"], defs["RM_ED_TRANSMITTING"], defs["RM_ED_BUSY"], defs["RM_ABI_VERSION"]) == ("-1", "1", "2", "5")
    assert (_lib.CHANNEL_OWN, _lib.ED_TRANSMITTING, _lib.ED_BUSY) == (-1, 1, 2)
    assert _lib.lib().rm_abi_version() == 5


def reference_scene(O):
    """10 000 nodes of configs[3]'s layout, the SINR medium with sigma 4 dB, one tick of 100 frames at t = 0."""
    from radio_sim_amd import workload as W
    n = 10_000
    src = W.make_nodes(n, 4)
    nd = O.NodeTable(n)
    nd.x, nd.y = src.x, src.y
    kind, kw = W.model_kwargs("logdist_sinr_overlap")
    assert kind == "logdist" and kw == dict(ld_sigma_db=4.0, ld_seed=0xC0FFEE, flags=1)
    params = {"ld_sigma_db": 4.0, "ld_seed": 0xC0FFEE, "ld_flags": 1}
    srcs = W.choose_sources(n, 100, 0xC0FFEE04, 0)
    return nd, params, srcs, nd.packets(srcs, 0, W.AIR_US)


def test_reference_scene_meets_its_conditions(O):
    nd, params, srcs, frames = reference_scene(O)
    energy, flags, counting = R.channel_energy(O, O.model(4, **params), nd, frames, 0, threshold=-90.0)
    assert (counting >= 1).mean() >= 0.90 and (counting >= 2).mean() >= 0.80 and (counting >= 4).mean() >= 0.50
    assert (energy >= -90.0).mean() >= 0.15 and (energy == -100.0).mean() >= 0.02
    assert int((flags & R.ED_TRANSMITTING != 0).sum()) == 100 and set(np.flatnonzero(flags & R.ED_TRANSMITTING)) == set(srcs.tolist())
    assert np.array_equal((flags & R.ED_BUSY) != 0, energy >= -90.0)
    assert energy.min() == -100.0 and np.all(energy[counting == 0] == -100.0) and np.all(energy[counting > 0] > -100.0)
    # the end of a span is exclusive
    e2, f2, c2 = R.channel_energy(O, O.model(4, **params), nd, frames, 8128, nodes=np.arange(50), threshold=-90.0)
    assert np.all(e2 == -100.0) and not f2.any() and not c2.any()
