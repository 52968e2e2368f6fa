"""The oracle's side of the deep Philox cases (tests/_deep.py), without a GPU: the cases are what
they claim, so that tests/test_gpu_deep_philox.py holds the device to a run that is still alive
at t = 600, on a late lattice, across the eps floor -- or, in group e, to one that absorbs after
the first turn.  These are conditions on the inputs, not tolerances: a seed that fails one is
replaced, the condition stays.  The records are the ones the GPU file uses (one oracle run per
replica for both)."""
import numpy as np
import pytest

from oracle import spgg_oracle as O
from tests import _deep as D
from tests import _record as R


def _ids(batches):
    return [b.name for b in batches]


@pytest.mark.parametrize("b", D.A + D.B + D.C + D.D + D.F, ids=_ids(D.A + D.B + D.C + D.D + D.F))
def test_no_replica_absorbs_and_both_strategies_live_at_the_end(b):
    for k, rec in enumerate(D.records(b)):
        assert rec.stop_iter == 0 and rec.last == D.T, (b.name, k, rec.stop_iter)
        nc = rec.value[1:D.T + 2, R.NCOOP]        # cooperators at the start of 1 .. T and after T
        assert (nc > 0).all() and (nc < rec.n).all(), (b.name, k)
        assert np.isfinite(rec.value).all() and np.isfinite(rec.final["Q"]).all(), (b.name, k)
        assert rec.rep_dyadic      # the int8 reputation path


@pytest.mark.parametrize("b", D.E, ids=_ids(D.E))
def test_late_absorption_after_the_first_turn(b):
    stops = D.e_stops(b)
    for k, rec in enumerate(D.records(b)):
        if k in stops:
            stop, coop = stops[k]
            assert D.CHUNK < rec.stop_iter < D.T, (b.name, k, rec.stop_iter)
            assert (rec.stop_iter, rec.value[rec.last, R.NCOOP]) == (stop, coop), (b.name, k, rec.stop_iter)
            assert {stop - 1, stop, stop + 1} <= set(rec.rows)
            assert rec.value[stop, R.SUMP] != 0.0      # its start record is on a float row
        else:
            assert rec.stop_iter == 0, (b.name, k, rec.stop_iter)
            assert 0 < rec.value[D.T + 1, R.NCOOP] < rec.n, (b.name, k)


def test_absorptions_at_all_c_and_at_all_d():
    ends = {coop for stops in D.E_STOPS.values() for _, coop in stops.values()}
    assert ends == {0, 18 * 18}


@pytest.mark.parametrize("b", D.A, ids=_ids(D.A))
def test_reputation_clip_is_the_minority_path_early_and_the_majority_path_late(b):
    """Share of agents with R at R_min or R_max after iteration 20 and after iteration 600."""
    p = D.records(b)[0].params
    early = D.share_at_bound(D.reputation_after(b, 0, 20), p)
    late = D.share_at_bound(D.reputation_after(b, 0, D.T), p)
    print(b.name, "share of R at a bound: t = 20 %.3f, t = 600 %.3f" % (early, late))
    assert early < 0.4 and late > 0.7, (b.name, early, late)


def test_case_a_covers_both_reward_paths_with_and_without_the_previous_rewards():
    rows = [b.rows[0] for b in D.A]
    unit = [r["reward_weight_payoff"] == 1.0 for r in rows]
    ni = [r["influence_factor"] != 0.0 for r in rows]
    assert {(True, True), (True, False), (False, True)} <= set(zip(unit, ni))
    assert all(b.L == 120 and not b.M2 and b.alg == "qlearning" and len(b.rows) == 1 for b in D.A)


def test_epsilon_reaches_its_floor_at_390():
    p = R.oracle_params(R.BASE, 30, D.T, False, "reputation", "qlearning")
    eps = O.epsilon_schedule(p, D.T + 1)[1:]    # eps[t - 1] = eps_t: what iteration t leaves (epsilon_history_final)
    assert eps[D.T_FLOOR - 2] > p.epsilon_min
    assert (eps[D.T_FLOOR - 1:] == p.epsilon_min).all()
    # Expected SARSA's target at the crossing: eps_{t-1} > eps_t = eps_min
    assert eps[D.T_FLOOR - 2] > eps[D.T_FLOOR - 1] == p.epsilon_min
    assert {D.T_FLOOR - 2, D.T_FLOOR - 1, D.T_FLOOR, D.T_FLOOR + 1, D.T_FLOOR + 2} <= D.ROWS
    assert {D.CHUNK - 1, D.CHUNK, D.CHUNK + 1, D.CHUNK + 2} <= D.ROWS
    # every case runs this schedule
    for b in [b for g in D.GROUPS.values() for b in g]:
        assert all(row[k] == R.BASE[k] for row in b.rows for k in ("epsilon", "epsilon_decay", "epsilon_min"))


def test_epsilon_history_is_the_oracle_runs_own():
    p = R.oracle_params(R.BASE, 12, 420, False, "reputation", "expected_sarsa")
    ds, fin = O.run(p, np.random.RandomState(3), collect_snapshots=False)
    assert fin["stop_iter"] == 0
    rec = R.exact_record(R.BASE, 12, 420, False, "reputation", "expected_sarsa", rs=np.random.RandomState(3), rows=())
    assert np.array_equal(D.epsilon_history(rec), ds["epsilon_history_final"])


def test_sparse_record_equals_the_full_record_on_its_rows():
    """One L = 30 replica, bit for bit: value, mag and pay_mag on ROWS, the integer slots and GMAX
    on every row, and nothing on the other rows."""
    b = D.D[2]
    k = 2
    sparse = D.records(b)[k]
    full = R.philox_record(b.L, D.T, b.rows[k], b.seeds[k], k, b.M2, b.state, b.alg)
    assert full.rows is None and sparse.rows == tuple(sorted(D.ROWS))
    on = sorted(D.ROWS)
    off = [t for t in range(D.T + 2) if t not in D.ROWS]
    every = list(R.COUNTERS) + [R.GMAX]
    floats = [s for s in range(R.NSTAT) if s not in every]
    for name in ("value", "mag"):
        f, s = getattr(full, name), getattr(sparse, name)
        assert np.array_equal(f[on], s[on]), name
        assert np.array_equal(f[:, every], s[:, every]), name
        assert not s[off][:, floats].any(), name
    assert np.array_equal(full.pay_mag[on], sparse.pay_mag[on]) and not sparse.pay_mag[off].any()
    assert full.value[on][:, floats].any(axis=0).all()        # (no float slot idle on these rows)
    assert (full.last, full.stop_iter, full.rep_units_max) == (sparse.last, sparse.stop_iter, sparse.rep_units_max)
    for key in ("S", "R", "Q"):
        assert np.array_equal(full.final[key], sparse.final[key]), key
    # the helper: all of the full record's own rows pass, and a wrong counter off ROWS is seen
    bound = R.bounds(sparse)
    assert not R.mismatches_on_rows(full.value, sparse, bound)
    assert R.mismatches_on_rows(full.value, full, R.bounds(full)) == R.mismatches(full.value, full, R.bounds(full)) == []
    t_off = 300 + 1
    assert t_off not in D.ROWS
    for slot in (R.SW_CD, R.GMAX, R.GC0 + 2):
        got = full.value.copy()
        got[t_off, slot] += 1.0
        assert [m[:2] for m in R.mismatches_on_rows(got, sparse, bound)] == [(t_off, R.SLOT_NAMES[slot])]
    got = full.value.copy()
    got[D.T_FLOOR, R.SUMQ_D] += 1e-6      # a float slot on a float row: far past its bound
    assert [m[:2] for m in R.mismatches_on_rows(got, sparse, bound)] == [(D.T_FLOOR, "SUMQ_D0")]
