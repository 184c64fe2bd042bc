"""CPU tier of the carry of a CSMA-CA gated batch: rm_csma_schedule_carry and rm_csma_carry_collect against
the Python restatement (tests/csma_carry_ref.py), the merge rule against the oracle's whole run, and the conditions that keep
tests/test_gpu_csma_carry.py from passing vacuously -- computed with the oracle alone."""
import numpy as np
import pytest

import cca_batch_ref as BR
import csma_carry_ref as KR
import csma_ref as SR
import energy_ref as R


def _params(rsa, p):
    return rsa.Engine.csma_params(p.max_backoffs, p.min_be, p.max_be, p.seed)


def _same_schedule(rsa, p, n_src, t_cca, carry, what):
    want = KR.schedule(p, n_src, t_cca, carry)
    n_exp, origin, attempt = rsa.Engine.csma_schedule_carry(_params(rsa, p), n_src, t_cca, carry)
    np.testing.assert_array_equal(n_exp, [len(s) for s in want], err_msg=what + ": n_exp")
    np.testing.assert_array_equal(origin, [o for s in want for o, _, _ in s], err_msg=what + ": origin")
    np.testing.assert_array_equal(attempt, [a for s in want for _, a, _ in s], err_msg=what + ": attempt")
    return want


def _scene(O, name):
    sc = BR.scene(O, name)
    ticks, p = SR.SCENES[name]
    return sc, p, [len(s) for s in sc.ticks[:ticks]], [sc.times(k)[1] for k in range(ticks)]


def _random_carry(rng, n, p, n_ticks, t0):
    rows = [(t0 - 1000 * int(rng.integers(1, 9)), int(rng.integers(0, 900)), int(rng.integers(0, 5000)), int(rng.integers(0, n_ticks + 3)),
             int(rng.integers(1, p.max_backoffs + 1))) for _ in range(n)]
    return KR.carry_list(rows)


def test_schedule_carry_matches_the_restatement(rsa, O):
    from radio_sim_amd import _lib
    rng = np.random.default_rng(5)
    for name in SR.SCENES:
        sc, p, n_src, t_cca = _scene(O, name)
        carry = _random_carry(rng, 300, p, len(n_src), t_cca[0])
        assert (carry["tick"] >= len(n_src)).any() and (carry["attempt"] == p.max_backoffs).any()
        want = _same_schedule(rsa, p, n_src, t_cca, carry, name)
        assert sum(1 for s in want for o, _, _ in s if o >= sum(n_src)) > 200
        # an empty carry list: rm_csma_schedule
        a = rsa.Engine.csma_schedule(_params(rsa, p), n_src, t_cca)
        for form in (None, carry[:0]):
            b = rsa.Engine.csma_schedule_carry(_params(rsa, p), n_src, t_cca, form)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
        # carried packets only
        _same_schedule(rsa, p, [0] * len(n_src), t_cca, carry, name + ", no own packets")
    # RM_MAX_BATCH ticks, max_be 8
    n_src = np.zeros(_lib.MAX_BATCH, dtype=np.int32)
    n_src[::25] = 40
    t_cca = 1000 * np.arange(_lib.MAX_BATCH, dtype=np.int64) + 128
    p = SR.Params(5, 6, 8, 2 ** 63 + 11)
    carry = _random_carry(rng, 500, p, _lib.MAX_BATCH, 128)
    want = _same_schedule(rsa, p, n_src, t_cca, carry, "max_be 8")
    total = sum(len(s) for s in want)
    with pytest.raises(rsa.RadioMediumError) as err:
        rsa.Engine.csma_schedule_carry(_params(rsa, p), n_src, t_cca, carry, cap=total - 1)
    assert err.value.code == _lib.RM_ERR_CAPACITY and err.value.total == total
    # the carry list's own refusals
    good = (128, 3, 7, 0, 1)
    for field, v in ((4, 0), (4, 6), (3, -1), (1, -1)):
        row = list(good)
        row[field] = v
        with pytest.raises(rsa.RadioMediumError) as err:
            rsa.Engine.csma_schedule_carry(_params(rsa, p), [3], [0], KR.carry_list([good, tuple(row)]))
        assert err.value.code == _lib.RM_ERR_INVALID, (field, v)
    with pytest.raises(rsa.RadioMediumError) as err:          # an attempt within 1 .. 5, but not within 1 .. max_backoffs
        rsa.Engine.csma_schedule_carry(_params(rsa, SR.Params(2, 1, 3, 0)), [3], [0], KR.carry_list([(128, 3, 7, 0, 3)]))
    assert err.value.code == _lib.RM_ERR_INVALID
    L = _lib.lib()
    cnt, tc, total = np.array([3], dtype=np.int32), np.array([0], dtype=np.int64), _lib.C.c_int64(0)
    for n_carry in (-1, 2):                                    # a negative count, a count without a list
        assert L.rm_csma_schedule_carry(_lib.C.byref(_params(rsa, p)), 1, cnt.ctypes.data, tc.ctypes.data, None, n_carry, None, None, None, 0,
                                        _lib.C.byref(total)) == _lib.RM_ERR_INVALID


@pytest.mark.parametrize("name,cut", [("multi", 6), ("multi", 4), ("ch16", 5)])
def test_a_cut_schedule_continues_the_whole(rsa, O, name, cut):
    """every chain of ticks 0 .. cut-1 that is scheduled past the cut, fed as a carry, reproduces ticks cut .. of the unsplit schedule slot
    by slot (the schedule alone: every attempt, made or not)"""
    sc, p, n_src, t_cca = _scene(O, name)
    whole = SR.schedule(p, n_src, t_cca)
    head = SR.schedule(p, n_src[:cut], t_cca[:cut])
    first = np.concatenate([[0], np.cumsum(n_src)])
    rows, ids = [], []
    for o, a, nxt in sorted(e for s in head for e in s if e[2] >= cut):
        b = int(np.searchsorted(first, o, side="right")) - 1
        rows.append((t_cca[b], o - int(first[b]), 0, nxt - cut, a + 1))
        ids.append(o)
    carry = KR.carry_list(rows)
    assert len(carry) > 100
    n_exp, origin, attempt = rsa.Engine.csma_schedule_carry(_params(rsa, p), n_src[cut:], t_cca[cut:], carry)
    np.testing.assert_array_equal(n_exp, [len(s) for s in whole[cut:]])
    n_own, before = sum(n_src[cut:]), int(first[cut])
    back = np.array([ids[o - n_own] if o >= n_own else before + o for o in origin])
    np.testing.assert_array_equal(back, [o for s in whole[cut:] for o, _, _ in s])
    np.testing.assert_array_equal(attempt, [a for s in whole[cut:] for _, a, _ in s])


def _split(O, name, cuts):
    """the oracle's whole run cut at `cuts`: per part (first, last, carry-in, its packets, own table, carried table)"""
    sc, p, n_src, t_cca = _scene(O, name)
    r = SR.run(O, name)
    edges = [0] + list(cuts) + [len(n_src)]
    parts = []
    for first, last in zip(edges[:-1], edges[1:]):
        carry, ids = KR.carry_at(r, first, t_cca)
        own, carried = KR.tables_of(r, first, last, ids, carry)
        parts.append((first, last, carry, ids, own, carried))
    return sc, r, t_cca, parts


@pytest.mark.parametrize("name,cuts", [("multi", (6,)), ("multi", (4, 8)), ("ch16", (5,))])
def test_collect_and_the_merge_rule(rsa, O, name, cuts):
    """rm_csma_carry_collect over the oracle's tables of every part gives the restatement's carry-out, which is what the whole run says
    the next cut carries; the merged parts are the whole run.  Too small a cap: RM_ERR_CAPACITY and the count."""
    from radio_sim_amd import _lib
    sc, r, t_cca, parts = _split(O, name, cuts)
    m = KR.Merge(len(r.status))
    for n, (first, last, carry, ids, own, carried) in enumerate(parts):
        lists = r.lists[first:last]
        want, who = KR.collect(lists, t_cca[first:last], carry, own, carried)
        got = rsa.Engine.csma_carry_collect(lists, t_cca[first:last], carry, own, carried)
        np.testing.assert_array_equal(got, want)
        nxt = m.part(first, sum(len(s) for s in lists), own, carried, who)
        if n + 1 < len(parts):
            np.testing.assert_array_equal(want, parts[n + 1][2], err_msg="the carry-out is not what the whole run carries over the cut")
            assert nxt == parts[n + 1][3] and len(want) > 50
            with pytest.raises(rsa.RadioMediumError) as err:
                rsa.Engine.csma_carry_collect(lists, t_cca[first:last], carry, own, carried, cap=len(want) - 1)
            assert err.value.code == _lib.RM_ERR_CAPACITY and err.value.count == len(want)
    want = r.outcome()
    want[3] = KR.whole_pkt(r, cuts)                            # (packet numbers: positions among the part's live slots)
    np.testing.assert_array_equal(m.outcome(), want)
    dead = sum(int(r.n_exp[first + b]) - len(a) for first, last, _, ids, _, _ in parts for b, a in enumerate(KR.live(r, first, last, ids)))
    print(name, cuts, "dead slots of the whole that the split does not have:", dead, "of", int(r.n_exp.sum()))
    assert dead >= 5
    np.testing.assert_array_equal(m.energy.view(np.uint64), r.energy.view(np.uint64))


def _fate(r, ids):
    st = r.status[np.array(ids, dtype=np.int64)]
    return int((st == SR.SENT).sum()), int((st == SR.FAILED).sum()), int((st == SR.PENDING).sum())


def test_multi_meets_its_conditions(O):
    sc, r, t_cca, parts = _split(O, "multi", (6,))
    carry, ids = parts[1][2], parts[1][3]
    sent, failed, pending = _fate(r, ids)
    behind = int((carry["tick"] >= 6).sum())
    print("multi cut 6: carried", len(ids), "sent", sent, "failed", failed, "pending again", pending, "next attempt behind part 2", behind)
    assert len(ids) >= 100 and sent >= 5 and failed >= 5 and pending >= 5 and behind >= 5
    _, _, _, three = _split(O, "multi", (4, 8))
    twice = len(set(three[1][3]) & set(three[2][3]))
    print("multi 4 / 4 / 4: carried twice", twice)
    assert twice >= 5


def test_ch16_meets_its_conditions(O):
    sc, r, t_cca, parts = _split(O, "ch16", (5,))
    ids = set(parts[1][3])
    sent, failed, pending = _fate(r, sorted(ids))
    lose = win = 0
    for T in range(5, len(r.lists)):
        kept_at, lost_to = {}, set()
        for i, (o, a, nxt) in enumerate(r.sched[T]):
            j = int(r.made[T][i])
            if j < 0:
                continue
            if r.kept[T][i] >= 0:
                kept_at[j] = i
            elif j in kept_at and r.slot_flags[T][i] == R.ED_TRANSMITTING:     # sensed a clear channel, an earlier slot of its radio won
                lost_to.add(kept_at[j])
                lose += o in ids
        win += sum(1 for i in lost_to if r.sched[T][i][0] in ids)
    print("ch16 cut 5: carried", len(ids), "sent", sent, "failed", failed, "pending", pending, "carried slots that lose first-wins", lose,
          "that win it", win)
    assert len(ids) >= 1024 and sent >= 5 and failed >= 5 and pending >= 5 and lose >= 5 and win >= 5
