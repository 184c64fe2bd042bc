"""CPU tier of the carrier-sense gated batch: the new calls at the boundary, and the conditions that keep
tests/test_gpu_cca_batch.py from passing vacuously -- computed with the oracle alone (tests/cca_ref.py, tests/cca_batch_ref.py)."""
import os
import re

import numpy as np
import pytest

import cca_batch_ref as BR
import energy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (scene, ticks run, the batches the GPU tests issue over them: [first, last) )
BATCHES = [("multi", 12, [(0, 12), (0, 5), (5, 12), (4, 12)]), ("ch16", 6, [(0, 6)]), ("chain", 4, [(0, 4)])]


def test_gated_batch_symbols_at_the_boundary(rsa):
    from radio_sim_amd import _lib
    text = open(os.path.join(ROOT, "include", "radiomedium_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("rm_batch_run_sources_cca", "rm_batch_run_sources_cca_device"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 12, name
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().rm_abi_version() == 5
    assert hasattr(rsa.Engine, "batch_run_sources_cca") and hasattr(rsa.Engine, "batch_run_sources_cca_device")
    assert "Batches are not gated" not in text


def test_no_new_environment_knob():
    src = os.path.join(ROOT, "radio-sim_amd", "csrc")
    for f in ("rm_api_cca.cpp", "rm_ccabatch.hip"):
        assert "getenv" not in open(os.path.join(src, f)).read(), f


@pytest.mark.parametrize("name,ticks,batches", BATCHES, ids=[b[0] for b in BATCHES])
def test_batches_meet_their_conditions(O, name, ticks, batches):
    sc, r = BR.scene(O, name), BR.run(O, name, ticks)
    for first, last in batches:
        what = "%s, ticks %d .. %d" % (name, first, last - 1)
        flags = np.concatenate(r.flags[first:last])
        real = np.concatenate(r.lists[first:last]) >= 0
        assert (flags[real] != 0).any() and (flags[real] == 0).any(), what + ": deferred and kept candidates"
        all_kept, window_only = BR.wrong_readings(O, sc, r, first, last)
        assert (np.concatenate(all_kept) != flags).any(), what + ": 'every earlier candidate kept' gives the same flags"
        assert (np.concatenate(window_only) != flags).any(), what + ": 'the window only' gives the same flags"
        # RM_ED_TRANSMITTING that only a frame of the same batch explains: set in truth, not with the window alone
        from_batch = (flags & R.ED_TRANSMITTING) & ~(np.concatenate(window_only) & R.ED_TRANSMITTING)
        if (first, last) == batches[0]:
            assert from_batch.any(), what + ": no RM_ED_TRANSMITTING from a frame of the same batch"
        print(what, "candidates", int(real.sum()), "deferred", int((flags[real] != 0).sum()), "differ from all-kept",
              int((np.concatenate(all_kept) != flags).sum()), "differ from window-only", int((np.concatenate(window_only) != flags).sum()),
              "transmitting from the batch", int(from_batch.astype(bool).sum()))


def test_the_hand_built_chain(O):
    sc, r = BR.scene(O, "chain"), BR.run(O, "chain", 4)
    at = lambda k, node: int(np.flatnonzero(r.lists[k] == node)[0])
    assert r.flags[0][at(0, sc.a)] == 0                                      # A is kept in tick 0
    assert r.flags[1][at(1, sc.b)] == R.ED_BUSY                              # B senses A: deferred
    assert r.flags[2][at(2, sc.c)] == 0                                      # C senses B, not A -- and B is not on the air: kept
    assert r.flags[3][at(3, sc.a)] & R.ED_TRANSMITTING                       # A again while its frame is live
    fb = r.flags[2][at(2, sc.b)]
    assert fb != 0 and not (fb & R.ED_TRANSMITTING)                          # B again: deferred in tick 1, so it is not transmitting
    all_kept, _ = BR.wrong_readings(O, sc, r, 0, 4)
    assert all_kept[2][at(2, sc.c)] & R.ED_BUSY                              # "everybody is on the air" defers C
    assert all_kept[2][at(2, sc.b)] & R.ED_TRANSMITTING                      # ... and finds B transmitting
