"""The frame error model without a device: known answers of the spec, the reference
(tests/errmodel_ref.py) against an independent evaluation, the draw, the library's host exports bit for bit against the
reference, and the conditions the scenes of tests/test_gpu_errmodel.py have to meet -- asserted for the reference alone."""
import ctypes as C
import math

import numpy as np
import pytest

import errmodel_ref as R

NAN = float("nan")
GRID_SINR = [-6.0 + 0.25 * i for i in range(65)]  # -6 .. +10 dB
GRID_AIR = (160, 1024, 4256)


def bits(x):
    return np.float64(x).view(np.uint64)


def test_known_answers_of_the_spec():
    # s = 0: every exponent is -0, acc = sum_{k>=2} (-1)^k C(16,k) = 15, ber = 0.5; det_log2(0.5) = -1; 100 bits
    assert R.psr(float("-inf"), 400) == 2.0 ** -100
    # 30 dB: every exponent is below -1022, det_exp2 gives 0, ber = 0, det_log2(1) = 0
    assert R.psr(30.0, 4064) == 1.0
    p = R.psr(NAN, 4064)
    assert p != p
    assert not (R.draw(0, 1, 0, 2) < p)  # a NaN psr never delivers
    for x in GRID_SINR[::4]:
        for a in GRID_AIR:
            assert bits(R.psr(x, 2 * a, us_per_bit=8.0)) == bits(R.psr(x, a, us_per_bit=4.0))
    # monotone where it matters, and a real transition: a 127-byte frame is lost at -3 dB and safe at +3 dB
    assert R.psr(-3.0, 4064) < 1e-6 and R.psr(3.0, 4064) > 0.9999
    assert R.psr(0.0, 160) > R.psr(0.0, 4064)  # the shorter frame survives more often


def test_psr_against_an_independent_evaluation():
    """math.exp / math.fsum / math.comb / ** instead of det_exp2, the running sum, the literals and det_log2.  The alternating sum
    cancels three to four digits near 0 dB.  Largest relative difference measured on the development machine: 1.645e-12 (at
    -4.75 dB, 4256 us); asserted: four times that, which covers libm differences between machines."""
    worst = 0.0
    for x in GRID_SINR:
        s = 10.0 ** (x / 10.0)
        b = (8.0 / 15.0) * (1.0 / 16.0) * math.fsum(((-1) ** k) * math.comb(16, k) * math.exp(20.0 * s * (1.0 / k - 1.0)) for k in range(2, 17))
        b = min(max(b, 0.0), 0.5)
        for air in GRID_AIR:
            want = (1.0 - b) ** (air / 4.0)
            worst = max(worst, abs(R.psr(x, air) - want) / want)
    print("largest relative difference: %.4g" % worst)
    assert worst <= 4 * 1.645e-12


def test_draw():
    assert R.draw(0, 1, 0, 2) != R.draw(0, 2, 0, 1)          # symmetric in nothing
    assert R.draw(0, 1, 0, 2) != R.draw(0, 1, 1, 2) and R.draw(0, 1, 0, 2) != R.draw(1, 1, 0, 2)
    rng = np.random.default_rng(5)
    u = np.array([R.draw(9, int(a), int(t), int(b)) for a, t, b in zip(rng.integers(0, 1 << 20, 100_000), rng.integers(0, 1 << 40, 100_000),
                                                                       rng.integers(0, 1 << 20, 100_000))])
    assert abs(u.mean() - 0.5) < 0.005 and u.min() > 0.0 and u.max() < 1.0
    # (seed 0, src 1, start 0, dst 2), step by step:
    #   mix64(0 + 0x9E3779B97F4A7C15)              = 0xE220A8397B1DCDAF   (SplitMix64's first output for seed 0)
    #   mix64(0xE220A8397B1DCDAF ^ 0)              = 0x48218226FF3CD4BF
    #   mix64(0x48218226FF3CD4BF ^ 0x0000000100000002) = 0x56135D49BAD8FD19
    #   u = ((h >> 12) + 0.5) * 2^-52 = (0x56135D49BAD8F + 0.5) / 2^52 = 0x1.584d7526eb63ep-2
    assert R.mix64(R.GOLDEN) == 0xE220A8397B1DCDAF
    assert R.draw_hash(0, 1, 0, 2) == 0x56135D49BAD8FD19
    assert R.draw(0, 1, 0, 2) == float.fromhex("0x1.584d7526eb63ep-2")


def test_host_exports_equal_the_reference_bit_for_bit(rsa):
    """rm_error_model_psr / rm_error_model_draw: csrc/rm_math.hpp as the host compiler builds it; no device needed"""
    from radio_sim_amd import _lib
    P = _lib.lib()
    e = rsa.ErrorModel()
    P.rm_error_model_defaults(C.byref(e), rsa.EM_OQPSK_250K)
    assert (e.kind, e.reserved, e.us_per_bit, e.seed) == (rsa.EM_OQPSK_250K, 0, 4.0, 0)
    for upb in (4.0, 8.0, 3.2):
        e.us_per_bit = upb
        for x in GRID_SINR + [float("-inf"), float("inf"), 18.4, 18.6, 30.0, -40.0]:
            for air in GRID_AIR + (0, 400, 8128):
                assert bits(P.rm_error_model_psr(C.byref(e), x, air)) == bits(R.psr(x, air, upb)), (x, air, upb)
    p = P.rm_error_model_psr(C.byref(e), NAN, 4064)
    assert p != p
    rng = np.random.default_rng(6)
    for seed in (0, 77, (1 << 64) - 1):
        e.seed = seed
        for a, t, b in zip(rng.integers(0, 1 << 31, 300), rng.integers(-5, 1 << 50, 300), rng.integers(0, 1 << 31, 300)):
            assert bits(P.rm_error_model_draw(C.byref(e), int(a), int(t), int(b))) == bits(R.draw(seed, int(a), int(t), int(b)))
    assert rsa.Engine.error_model_psr(0.5, 4064) == R.psr(0.5, 4064) and rsa.Engine.error_model_draw(1, 0, 2) == R.draw(0, 1, 0, 2)
    e.kind = rsa.EM_NONE
    assert P.rm_error_model_psr(C.byref(e), -20.0, 4064) == 1.0


def _scene_results(name):
    if name == "lone":
        nd, srcs, start, air = R.scene_lone()
        return [R.Replay(nd).tick(0, srcs, start, air)]
    if name == "serial":
        nd, srcs, starts, _, air = R.scene_serial()
        rep = R.Replay(nd)
        return [rep.tick(int(s), [q], int(s), air) for q, s in zip(srcs, starts)]
    nd, lists, starts, air = R.scene_batch(name == "overlap")
    rep = R.Replay(nd)
    return [rep.tick(s, l, s, air) for l, s in zip(lists, starts)]


@pytest.mark.parametrize("name", ["lone", "serial", "batch", "overlap"])
def test_scene_conditions_hold_for_the_reference_alone(name):
    """among the oracle's RM_DELIVERED links at least 200 with 0.05 < psr < 0.95, at least 50 flipped, at least 50 of the 200
    kept, and a link flipped in a packet whose other links are kept: the GPU tests cannot pass vacuously"""
    res = _scene_results(name)
    trans, flipped, kept, mixed = R.scene_conditions(res)
    print(name, trans, flipped, kept, mixed)
    assert trans >= 200 and flipped >= 50 and kept >= 50 and mixed >= 1
    if name in ("batch", "overlap"):
        counts = [r.count for r, _ in res]
        assert counts[1] == 0 and max(counts) > 16384 and any(c % 64 for c in counts)
        assert all(r.pkt_offset[q] == r.pkt_offset[q + 1] for r, _ in res[2:3] for q in (0, 7, 47))  # the padding entries
