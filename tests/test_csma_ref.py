"""CPU tier of the CSMA-CA gated batch: rm_csma_schedule against the Python restatement of the schedule, and the
conditions that keep tests/test_gpu_csma.py from passing vacuously -- computed with the oracle alone (tests/csma_ref.py)."""
import numpy as np
import pytest

import cca_batch_ref as BR
import csma_ref as SR
import energy_ref as R


def _params(rsa, p, reserved=None):
    return rsa.Engine.csma_params(p.max_backoffs, p.min_be, p.max_be, p.seed, reserved)


def _same_schedule(rsa, p, n_src, t_cca, what):
    want = SR.schedule(p, n_src, t_cca)
    n_exp, origin, attempt = rsa.Engine.csma_schedule(_params(rsa, p), n_src, t_cca)
    np.testing.assert_array_equal(n_exp, [len(s) for s in want], err_msg=what + ": n_exp")
    np.testing.assert_array_equal(origin, [o for s in want for o, _, _ in s], err_msg=what + ": origin")
    np.testing.assert_array_equal(attempt, [a for s in want for _, a, _ in s], err_msg=what + ": attempt")
    return n_exp, origin, attempt


def test_schedule_matches_the_restatement(rsa, O):
    from radio_sim_amd import _lib
    for name, (ticks, p) in SR.SCENES.items():
        sc = BR.scene(O, name)
        n_src = [len(s) for s in sc.ticks[:ticks]]
        t_cca = [sc.times(k)[1] for k in range(ticks)]
        n_exp, origin, attempt = _same_schedule(rsa, p, n_src, t_cca, name)
        assert n_exp.sum() > sum(n_src) and attempt.max() == p.max_backoffs
        # max_backoffs = 0: the identity
        n_exp, origin, attempt = _same_schedule(rsa, SR.Params(0, p.min_be, p.max_be, p.seed), n_src, t_cca, name + ", no retries")
        np.testing.assert_array_equal(n_exp, n_src)
        np.testing.assert_array_equal(origin, np.arange(sum(n_src)))
        assert not attempt.any()
        # min_be = max_be = 0: every retry is in the next tick
        n_exp, origin, attempt = _same_schedule(rsa, SR.Params(3, 0, 0, 5), n_src, t_cca, name + ", BE 0")
        np.testing.assert_array_equal(n_exp, [sum(n_src[max(0, k - 3):k + 1]) for k in range(ticks)])
    # max_be = 8 over RM_MAX_BATCH ticks of which 21 have candidates (and some have none and receive retries)
    n_src = np.zeros(_lib.MAX_BATCH, dtype=np.int32)
    n_src[::25] = 40
    assert (n_src > 0).sum() == 21
    t_cca = 1000 * np.arange(_lib.MAX_BATCH, dtype=np.int64) + 128
    p = SR.Params(5, 6, 8, 2 ** 63 + 11)
    n_exp, origin, attempt = _same_schedule(rsa, p, n_src, t_cca, "max_be 8")
    assert ((n_src == 0) & (n_exp > 0)).sum() > 100 and attempt.max() == 5
    # defaults, and a negative sample time (the hash takes its two's complement)
    d = rsa.Engine.csma_params()
    assert (d.max_backoffs, d.min_be, d.max_be, d.reserved, d.seed) == (4, 3, 5, 0, 0)
    _same_schedule(rsa, SR.Params(), [30, 0, 30, 7], [-5000, -4000, -3000, 90], "defaults")
    # cap too small: RM_ERR_CAPACITY with *total set
    with pytest.raises(rsa.RadioMediumError) as err:
        rsa.Engine.csma_schedule(_params(rsa, p), n_src, t_cca, cap=int(n_exp.sum()) - 1)
    assert err.value.code == _lib.RM_ERR_CAPACITY and err.value.total == n_exp.sum()
    # parameters out of range, reserved != 0
    for bad in (SR.Params(6, 1, 3, 0), SR.Params(-1, 1, 3, 0), SR.Params(2, 4, 3, 0), SR.Params(2, 0, 9, 0), SR.Params(2, -1, 3, 0)):
        with pytest.raises(rsa.RadioMediumError) as err:
            rsa.Engine.csma_schedule(_params(rsa, bad), [3], [0])
        assert err.value.code == _lib.RM_ERR_INVALID
    with pytest.raises(rsa.RadioMediumError) as err:
        rsa.Engine.csma_schedule(_params(rsa, SR.Params(), reserved=1), [3], [0])
    assert err.value.code == _lib.RM_ERR_INVALID


def _counts(r, p):
    sent = [int(((r.status == SR.SENT) & (r.attempts == a + 1)).sum()) for a in range(p.max_backoffs + 1)]
    return sent, int((r.status == SR.FAILED).sum()), int((r.status == SR.PENDING).sum())


def test_multi_meets_its_conditions(O):
    r = SR.run(O, "multi")
    p = SR.SCENES["multi"][1]
    sent, failed, pending = _counts(r, p)
    print("multi: sent at attempts", sent, "failed", failed, "pending", pending, "sibling losses", r.sibling_losses, "largest n_exp", r.n_exp.max())
    assert all(s >= 1 for s in sent) and sum(sent[1:]) >= 20
    assert failed >= 5 and pending >= 5 and r.sibling_losses >= 5


def test_ch16_meets_its_conditions(O):
    r = SR.run(O, "ch16")
    p = SR.SCENES["ch16"][1]
    sent, failed, pending = _counts(r, p)
    print("ch16: sent at attempts", sent, "failed", failed, "pending", pending, "sibling losses", r.sibling_losses, "largest n_exp", r.n_exp.max())
    assert r.sibling_losses >= 100 and r.n_exp.max() > 2048
    # a kept slot at a position >= 1024 (the resolve pass's second stride) whose frame a later tick senses: without it, some later
    # slot's energy changes
    sc = BR.scene(O, "ch16")
    found = False
    for T in range(len(r.n_exp) - 1):
        late = np.flatnonzero(r.kept[T][1024:] >= 0) + 1024
        if r.n_exp[T] <= 1024 or not len(late):
            continue
        src = r.kept[T][late]
        nxt = r.made[T + 1]
        ok = np.flatnonzero(nxt >= 0)
        frames = r.onair[T]
        without = frames[~(np.isin(frames["src"], src) & (frames["start_us"] == sc.times(T)[2]))]
        assert len(without) == len(frames) - len(late)
        e_with = R.channel_energy(O, sc.model(O), sc.nd, frames, sc.times(T + 1)[1], nodes=nxt[ok], threshold=sc.threshold)[0]
        e_without = R.channel_energy(O, sc.model(O), sc.nd, without, sc.times(T + 1)[1], nodes=nxt[ok], threshold=sc.threshold)[0]
        found = found or bool((e_with != e_without).any())
    assert found


@pytest.mark.parametrize("name", ["multi", "ch16"])
def test_wrong_readings_differ(O, name):
    r = SR.run(O, name)
    for kw, what in ((dict(first_wins=False), "a sibling is kept too"), (dict(phantom=True), "deferred attempts sensed as on the air")):
        w = SR.run(O, name, **kw)
        assert (w.outcome() != r.outcome()).any(), "%s: '%s' gives the same outcome" % (name, what)
        print(name, what, "packets that differ:", int((w.outcome() != r.outcome()).any(axis=0).sum()))


def test_the_hand_built_chain(O):
    c = SR.chain_run(O)
    r, (a0, b1, c2, a3) = c.run, c.at
    # A in tick 0: nothing on the air -> sent at once, the last slot of its tick's list
    assert (r.status[a0], r.attempts[a0], r.tick[a0], r.pkt[a0], r.flags[a0]) == (SR.SENT, 1, 0, len(c.lists[0]) - 1, 0)
    # B in tick 1 senses A (on the air until 1160, the sample is at 1128): deferred; its retry in tick 2 finds A gone: sent there, in a
    # slot behind the tick's own entries
    assert (r.status[b1], r.attempts[b1], r.tick[b1], r.flags[b1]) == (SR.SENT, 2, 2, 0)
    assert r.pkt[b1] >= len(c.lists[2]) and r.kept[2][r.pkt[b1]] == c.sc.b
    assert r.slot_flags[1][len(c.lists[1]) - 1] == R.ED_BUSY
    # C in tick 2: A has left the air, B's retry starts in this very tick (slots of one tick never see each other): sent at once
    assert (r.status[c2], r.attempts[c2], r.tick[c2], r.flags[c2]) == (SR.SENT, 1, 2, 0)
    # A in tick 3 senses B's frame of tick 2 (the link is the one over which B sensed A): deferred, and its retry falls at tick 4,
    # behind the batch: pending
    assert (r.status[a3], r.attempts[a3], r.tick[a3], r.pkt[a3]) == (SR.PENDING, 1, 4, -1) and r.flags[a3] & R.ED_BUSY
