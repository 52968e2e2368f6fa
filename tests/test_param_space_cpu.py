"""The oracle's side of the parameter-space tests (tests/test_gpu_param_space.py), without a GPU.

The rows are fixed by seed, so everything here is deterministic.  Each condition is asserted on the
oracle alone: a batch whose replicas blew up, absorbed at once or lost a strategy would let the
device pass by computing nothing.  The kernel's division (div_uniform, spgg_device.h) is held to
IEEE division in exact rational arithmetic on every quotient the rows can reach."""
import numpy as np
import pytest

from oracle import spgg_oracle as O
from tests import _params as P
from tests import _record as R

BATCHES = P.step_batches()
ROWS = P.all_rows()
RANGES = dict(r=(0.5, 6), c=(0.5, 2), cost=(0, 2), alpha=(0.05, 1), gamma=(0, 1), epsilon=(0.05, 1),
              epsilon_decay=(0.9, 1), epsilon_min=(0, 0.2), lambda_epsilon=(1e-6, 1), reward_weight_payoff=(0, 1),
              alg_alpha=(0.05, 1), alg_gamma=(0, 1))


def _id(b):
    return "-".join(str(x) for x in (b.name, b.rng, b.L, b.alg, "M2" if b.M2 else "M1", b.state))


# ---- the rows themselves ------------------------------------------------------------------------------
def test_rows_are_seeded_and_inside_their_ranges():
    a, b = P.rows(7, 40), P.rows(7, 40)
    assert a == b and a != P.rows(8, 40)
    assert a[:10] == P.rows(7, 10)                  # a row does not depend on how many follow it
    for i, row in enumerate(a):
        assert set(row) == set(P.ROW_KEYS)
        for k, (lo, hi) in RANGES.items():
            assert lo <= row[k] <= hi, (i, k, row[k])
        assert (row["influence_factor"] == 0.0) == (i % 4 == 3)
        assert row["influence_factor"] == 0.0 or 0.1 <= row["influence_factor"] <= 3
        assert (P.unit_of(row) is None) == (i % 2 == 1)
        assert row["alg_alpha"] != row["alpha"] and row["alg_gamma"] != row["gamma"]
    for row in P.rows(9, 20, "dyadic"):
        u = P.unit_of(row)
        assert u in P.UNITS
        ks = [row[k] / u for k in ("rep_gain_C", "delta_R_D", "R_min", "R_max")]
        assert all(k == int(k) for k in ks) and -128 <= ks[2] <= 0 <= ks[3] <= 127, ks
    for row in P.rows(9, 20, "free"):
        assert P.unit_of(row) is None
        assert 0.1 <= row["rep_gain_C"] <= 2 and 0.1 <= row["delta_R_D"] <= 2
        assert 1 <= row["R_max"] <= 12 and 1 <= -row["R_min"] <= 12


def test_edge_rows_change_base_in_one_place():
    assert len(P.EDGE) == 23
    for name, row in P.EDGE.items():
        assert set(row) == set(P.ROW_KEYS), name
        assert row["alg_alpha"] is None and row["alg_gamma"] is None
    one = {n: {k for k in R.PARAM_KEYS if r[k] != R.BASE[k]} for n, r in P.EDGE.items()}
    assert one["always_explore"] == {"epsilon", "epsilon_decay"} and one["never_explore"] == {"epsilon", "epsilon_min"}
    assert one["rep_bounds_0"] == {"R_min", "R_max"}
    assert all(len(d) == 1 for n, d in one.items()
               if not n.startswith(("always", "never", "rep_bounds", "rep_smallest", "rep_int8")))
    # the smallest-unit row (bounds +-0.125) reaches +128 units: not an int8 row; its variant is, at the same unit
    assert P.unit_of(P.EDGE["rep_smallest_unit"]) is None
    assert P.unit_of(P.EDGE_INT8["rep_smallest_unit_int8"]) == 2.0 ** -10
    assert P.unit_of(P.EDGE["rep_int8_limits"]) == 1.0
    assert all(P.unit_of(r) is not None for r in P.EDGE_INT8.values())
    assert list(P.EDGE_INT8)[list(P.EDGE).index("rep_smallest_unit")] == "rep_smallest_unit_int8"


def test_dyadic_batches_hold_several_units():
    for b in BATCHES:
        units = [P.unit_of(row) for row in b.rows]
        if all(u is not None for u in units) and not b.name.startswith(("c-", "h")):
            assert len(set(units)) >= 3, (_id(b), units)
    assert all(P.unit_of(r) is not None for r in P.B_ROWS["dyadic"])
    assert any(P.unit_of(r) is None for r in P.B_ROWS["mixed"]) and any(P.unit_of(r) for r in P.B_ROWS["mixed"])
    for n, rows_ in P.E_ROWS.items():
        kappas = [r["influence_factor"] for r in rows_]
        assert len(rows_) == n and 0.0 in kappas and any(kappas)


# ---- every stepped batch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("b", BATCHES, ids=_id)
def test_batch_is_finite_and_alive(b):
    assert b.L in R.GPU_LATTICES
    recs = P.records(b)
    for k, rec in enumerate(recs):
        assert np.isfinite(rec.value).all() and np.isfinite(rec.mag).all() and np.isfinite(rec.pay_mag).all(), k
        fin = rec.final
        assert all(np.isfinite(fin[x]).all() for x in ("Q", "R", "P")), k
        if fin["tables"] is not None:
            assert np.isfinite(fin["tables"][0]).all() and np.isfinite(fin["tables"][1]).all(), k
    early = [k for k, rec in enumerate(recs) if 0 < rec.stop_iter < b.T]
    assert 8 * len(early) <= len(recs), early
    alive = [k for k, rec in enumerate(recs)
             if not rec.stop_iter and 0 < np.sum(rec.final["S"] == 0) < rec.n]
    assert alive, "no replica ends with both strategies"


def test_epsilon_schedules_end_in_different_strategies():
    for rng in P.RNGS:
        b = P.batch_h(rng)
        assert len(set(b.seeds)) == 1
        for i, ri in enumerate(b.rows):
            for rj in b.rows[:i]:
                assert {k for k in P.ROW_KEYS if ri[k] != rj[k]} <= {"epsilon", "epsilon_decay", "epsilon_min"}
        fin = [rec.final["S"] for rec in P.records(b)]
        for i in range(len(fin)):
            for j in range(i):
                assert not np.array_equal(fin[i], fin[j]), (rng, i, j)


def test_sweep_model_is_the_runners():
    from spgg_amd import sweep
    assert {k: sweep.RUNNER_MODEL[k] for k in P.RUNNER_MODEL} == P.RUNNER_MODEL
    p8 = P.G_TUPLES[2]
    rep = sweep._replica(p8, dict(sweep.RUNNER_MODEL), 5)
    assert {k: getattr(rep, k) for k in P.ROW_KEYS} == P.sweep_row(p8)


def test_sweep_tuples_share_one_engine_and_stay_alive():
    assert len({(p[2], p[6], p[7]) for p in P.G_TUPLES}) == 1 and len(P.G_TUPLES) == 8
    for f in (0, 1, 3, 4, 5):       # r, kappa, alpha, w_P, rep_gain_C
        assert len({p[f] for p in P.G_TUPLES}) >= 4, f
    assert P.G_SHAPE["L"] in R.GPU_LATTICES
    early, alive = 0, 0
    for p8, seed in zip(P.G_TUPLES, P.G_SEEDS):
        op = P.oracle_params(P.sweep_row(p8), P.G_SHAPE["L"], P.G_SHAPE["iterations"], p8[2], p8[6], p8[7])
        ds, fin = O.run(op, np.random.RandomState(seed), collect_snapshots=False)
        assert np.isfinite(fin["Q"]).all() and np.isfinite(fin["R"]).all()
        early += 0 < fin["stop_iter"] < op.iterations
        alive += fin["stop_iter"] == 0 and 0 < np.sum(fin["S"] == 0) < fin["S"].size
    assert 8 * early <= len(P.G_TUPLES) and alive


# ---- a: the payoff lattices --------------------------------------------------------------------------------
@pytest.mark.parametrize("L", P.A_SIDES)
def test_payoff_lattices_read_every_reachable_table_entry(L):
    S = P.payoff_strategies(L, len(P.A_ROWS))
    assert len(S) == 48 and all(s.shape == (L, L) and set(np.unique(s)) <= {0, 1} for s in S)
    assert not S[-4].any() and S[-3].all()
    dens = [s.mean() for s in S[:-4]]
    assert min(dens) < 0.15 and max(dens) > 0.85
    reads = set().union(*(P.table_reads(s) for s in S))
    # pay_c[0] and pay_d[5] cannot be read: an agent is a member of each of its five groups
    assert reads == {(0, N) for N in range(1, 6)} | {(1, N) for N in range(0, 5)}
    for k, row in enumerate(P.A_ROWS):
        assert np.isfinite(O.payoff(S[k], P.oracle_params(row, L, 1, True, "reputation", "qlearning"))).all()


def test_table_reads_counts_the_groups_the_oracle_sums():
    """table_reads against a direct evaluation: with the table entries 10^N (C) and -10^N (D) the
    digits of the oracle's unnormalised total spell out which entries it added."""
    rs = np.random.RandomState(3)
    S = (rs.rand(7, 7) < 0.5).astype(np.int64)
    N0 = O.sum5((S == 0).astype(int))
    want = set()
    for g in [None, (1, 0), (-1, 0), (1, 1), (-1, 1)]:
        S0 = (S == 0).astype(int)
        N = O.sum5(S0 if g is None else np.roll(S0, *g))
        want |= {(int(s), int(n)) for s, n in zip(S.ravel(), N.ravel())}
    assert P.table_reads(S) == want and N0.max() <= 5


# ---- the kernel's division -------------------------------------------------------------------------------------
def test_division_model_is_ieee_division_on_random_pairs():
    rs = np.random.RandomState(11)
    x = rs.uniform(-40, 40, 3000) * 10.0 ** rs.randint(-6, 3, 3000)
    d = rs.uniform(0.1, 60, 3000)
    assert all(P.div_uniform(float(a), float(b)) == float(a) / float(b) for a, b in zip(x, d))
    assert P.div_uniform(0.0, 3.0) == 0.0 and P.div_uniform(7.0, 7.0) == 1.0


@pytest.mark.parametrize("name", sorted(ROWS))
def test_division_model_on_every_payoff_total(name):
    x, d = P.payoff_quotients(ROWS[name])
    assert d != 0 and np.isfinite(x).all() and x.size >= 30
    bad = [(float(v), d) for v in x if P.div_uniform(float(v), d) != float(v) / d]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_division_model_on_the_neighbour_influence_quotients(name):
    row = ROWS[name]
    seen = 0
    for x, d in P.ni_quotients(row):
        assert d > 0 and np.isfinite(d)
        seen += x.size
        bad = [(float(v), d) for v in x if P.div_uniform(float(v), float(d)) != float(v) / float(d)]
        assert not bad, bad[:5]
    assert seen >= 5
