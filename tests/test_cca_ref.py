"""CPU tier of the carrier-sense gated tick: the new calls at the boundary, and the conditions of the
scenes tests/test_gpu_cca.py runs -- computed with the oracle alone (tests/cca_ref.py), so that a later edit of a scene cannot
hollow the GPU tests out without this file noticing."""
import os
import re

import numpy as np
import pytest

import cca_ref as CR
import energy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gated_tick_symbols_at_the_boundary(rsa):
    from radio_sim_amd import _lib
    text = open(os.path.join(ROOT, "include", "radiomedium_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rm_tick_run_sources_cca", "rm_tick_run_sources_cca_device"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 11, name
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().rm_abi_version() == 5
    assert hasattr(rsa.Engine, "tick_run_sources_cca") and hasattr(rsa.Engine, "tick_run_sources_cca_device")


def test_no_new_environment_knob():
    src = os.path.join(ROOT, "radio-sim_amd", "csrc")
    for f in ("rm_api_cca.cpp", "rm_energy.hip", "rm_api_energy.cpp"):
        assert "getenv" not in open(os.path.join(src, f)).read(), f


@pytest.mark.parametrize("name", ["multi", "ch16"])
def test_scene_meets_its_conditions(O, name):
    sc = CR.Scene(O, name)
    mdl = sc.model(O)
    chain, alone = CR.Chain(O, sc.nd, mdl), 0
    n_cand = n_def = n_tx_only = n_busy_only = n_pad = from_the_air = 0
    for k, src in enumerate(sc.ticks):
        t0, tc, ts = sc.times(k)
        flags, energy, exp = chain.gated_tick(t0, src, ts, CR.AIR, tc, sc.threshold)
        real = src >= 0
        n_pad += int((~real).sum())
        assert not flags[~real].any() and np.all(np.isnan(energy[~real])) and not np.isnan(energy[real]).any()
        n_cand += int(real.sum())
        n_def += int((flags[real] != 0).sum())
        n_tx_only += int((flags == R.ED_TRANSMITTING).sum())
        n_busy_only += int((flags == R.ED_BUSY).sum())
        assert np.array_equal(exp.slots, np.flatnonzero(real & (flags == 0)))
        # kept frames that are heard and interfered BY A FRAME STILL ON THE AIR: interfered here, not among the tick's own frames alone
        if exp.raw is not None:
            own = O.tick_mt(mdl, sc.nd, exp.new, cap=1 << 22)
            assert own.count == exp.count and np.array_equal(own.dst, exp.raw.dst)     # (the heard links do not depend on the air)
            from_the_air += int(((exp.raw.verdict == O.INTERFERED) & (own.verdict != O.INTERFERED)).sum())
    assert n_pad > 0
    assert 0.10 * n_cand <= n_def <= 0.90 * n_cand, (n_def, n_cand)
    assert n_tx_only >= 1 and n_busy_only >= 1, (n_tx_only, n_busy_only)
    assert from_the_air >= 1
    print(name, "candidates", n_cand, "deferred", n_def, "tx only", n_tx_only, "busy only", n_busy_only, "interfered from the air", from_the_air)
