"""The step kernel held to the oracle across its parameter space.

tests/test_gpu_record.py varies the launch layout over a handful of parameter points; here the
layout stays small and the parameters move: every field of spgg_rep_params different in every
replica of a batch (tests/_params.rows: payoff table, both learning rates and discounts, the eps
schedule, kappa, lambda_epsilon, the reward weights, the reputation quadruple and its int8 unit),
the named edge rows (tests/_params.EDGE), the replica permutation of a launch forced, replica
groups, persistent launches, the sweep runner's own batching, and spgg_payoff on its own.

Every stepped batch goes through test_gpu_record's _check: S, R, Q, Double-Q's two tables and the
stop iteration bit-equal, all 34 record slots under tests/_record.bounds.  A replica that read
another replica's parameter -- replica 0's, its group's first, the logical instead of the permuted
index -- computes another run and fails there.  tests/test_param_space_cpu.py holds the oracle's
side: every batch finite, at most one replica in eight absorbed early, both strategies alive."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import spgg_oracle as O  # noqa: E402
from spgg_amd import sweep  # noqa: E402
from spgg_amd.engine import BatchEngine, InitState  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402
from tests import _params as P  # noqa: E402
from tests import _record as R  # noqa: E402
from tests.test_gpu_parity import APPROX, FLOAT_TOL  # noqa: E402
from tests.test_gpu_record import _check, _force, _run  # noqa: E402


def _reps(b):
    return [P.replica_params(row, s) for row, s in zip(b.rows, b.seeds)]


def _go(b, look=None, **engine_kw):
    """Run batch b to its end and hold it to its exact records; the folded record array."""
    return _run(b.L, b.T, _reps(b), b.M2, b.state, b.alg, b.rng, P.records(b), look, **engine_kw)


# ---- a. payoff alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("L", P.A_SIDES)
def test_payoff_alone(L, streams, monkeypatch):
    """spgg_payoff (SPGG.P, run()'s return value) of 48 replicas, replica k with row k's payoff
    table on lattice k of payoff_strategies: every element bit-equal to the oracle's.  L = 5: the
    13-cell stencil wraps onto itself; three replica groups: each group's slice of the parameters."""
    _force(monkeypatch)
    S = P.payoff_strategies(L, len(P.A_ROWS))
    reads = set().union(*(P.table_reads(s) for s in S))
    # a cooperator sits in each of its five groups (N >= 1), a defector leaves each at N <= 4: those two
    # entries are never read, every other one is
    assert reads == {(0, N) for N in range(1, 6)} | {(1, N) for N in range(0, 5)}, sorted(reads)
    rs = np.random.RandomState(L)
    init = [InitState(Q=rs.uniform(-0.01, 0.01, size=(L, L, 2, 2)), S=s) for s in S]
    reps = [P.replica_params(row, k) for k, row in enumerate(P.A_ROWS)]
    eng = BatchEngine(L, 1, reps, use_second_order=True, rng="philox", init=init, streams=streams)
    try:
        assert eng.G == streams
        got = eng.payoff_at(1)
    finally:
        eng.close()
    for k, row in enumerate(P.A_ROWS):
        want = O.payoff(S[k], P.oracle_params(row, L, 1, True, "reputation", "qlearning"))
        assert np.isfinite(want).all()
        assert np.array_equal(got[k], want), (k, row, int(np.sum(got[k] != want)))


# ---- b. every field different in every replica ----------------------------------------------------------
@pytest.mark.parametrize("apt", ["1", "max"])
@pytest.mark.parametrize("rng", P.RNGS)
@pytest.mark.parametrize("M2,state", P.CONFIGS_B)
@pytest.mark.parametrize("alg", P.ALGS)
@pytest.mark.parametrize("kind", ["dyadic", "mixed"])
def test_every_field_differs_in_every_replica(kind, alg, M2, state, rng, apt, monkeypatch):
    _force(monkeypatch, SPGG_APT=apt)

    def look(eng):      # all dyadic: the int8 lattice with a unit per replica; one free row: f64 planes
        assert eng.rep_int8 == (kind == "dyadic")
        if kind == "dyadic":
            assert len(set(eng.rep_units.tolist())) >= 3

    _go(P.batch_b(kind, alg, M2, state, rng), look)


# ---- c. edge rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", P.RNGS)
@pytest.mark.parametrize("alg", ["qlearning", "expected_sarsa"])
@pytest.mark.parametrize("kind", ["edge", "int8"])
def test_edge_rows(kind, alg, rng, monkeypatch):
    """EDGE as one batch (its +-128-unit row puts the batch on f64 reputation planes), and the same
    rows with that bound one unit lower on the int8 lattice."""
    _force(monkeypatch)

    def look(eng):
        assert eng.rep_int8 == (kind == "int8")

    _go(P.batch_c(kind, alg, rng), look)


# ---- d. compile-time widths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M2,state,alg,kind", P.CTW_ROWS)
def test_width_20_tiles(M2, state, alg, kind, monkeypatch):
    _force(monkeypatch, SPGG_APT="2")

    def look(eng):
        assert eng.tile[0] == 20, eng.tile
        assert eng.rep_int8 == (kind == "dyadic")

    _go(P.batch_d(60, M2, state, alg, kind), look)


@pytest.mark.parametrize("M2,state,alg,kind", P.CTW_ROWS)
def test_width_40_tiles(M2, state, alg, kind, monkeypatch):
    _force(monkeypatch, SPGG_APT="max")

    def look(eng):
        assert eng.tile == (40, 24), eng.tile
        assert eng.rep_int8 == (kind == "dyadic")

    _go(P.batch_d(120, M2, state, alg, kind), look)


# ---- e. the replica permutation of a launch ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 11])
def test_replica_permutation(n, monkeypatch):
    """Logical replica j of a launch runs replica (j * stride) % n: stride 3, a stride that is not
    coprime to n (the library falls back to 1), n - 1 for n = 7, and the library's own choice --
    every run against the oracle, and their record arrays bit-equal to each other."""
    b = P.batch_e(n)
    kappas = [row["influence_factor"] for row in b.rows]
    assert 0.0 in kappas and any(kappas)
    runs = {}
    for stride in [None, "3", str(2 * n)] + (["6"] if n == 7 else []):
        _force(monkeypatch)
        if stride is None:
            monkeypatch.delenv("SPGG_REP_STRIDE", raising=False)
        else:
            monkeypatch.setenv("SPGG_REP_STRIDE", stride)
        runs[stride] = _go(b, streams=1)
    monkeypatch.delenv("SPGG_REP_STRIDE", raising=False)
    for stride, st in runs.items():
        assert np.array_equal(st, runs[None]), stride


# ---- f. groups and persistence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 3])
def test_replica_groups(streams, monkeypatch):
    """b's dyadic batch in one and in three contexts: each group's slice of params, eps and units."""
    _force(monkeypatch)

    def look(eng):
        assert eng.G == streams and eng.rep_int8

    _go(P.batch_f(18), look, streams=streams)


def test_persistent_launches(monkeypatch):
    """The same rows at L = 60, the smallest lattice with a persistent launch (below it the library
    has no compile-time-width tiling), in step(5), step(T - 5)."""
    _force(monkeypatch, SPGG_PERSIST="1", SPGG_APT="2")
    b = P.batch_f(60)
    eng = BatchEngine(b.L, b.T, _reps(b), use_second_order=b.M2, state_representation=b.state, rng=b.rng,
                      algorithm=b.alg)
    try:
        assert eng.persistent and eng.rep_int8, (eng.persist_capacity, eng.tile)
        eng.step(5)
        eng.step(b.T - 5)
        eng.flush()
        _check(eng, P.records(b))
    finally:
        eng.close()


# ---- g. the sweep's own batching -----------------------------------------------------------------------------------------
def test_sweep_batches_differing_tuples(tmp_path, monkeypatch):
    """sweep.run_batch puts tuples that differ in alpha, w_P, rep_gain_C, r and kappa into one
    BatchEngine: every dataset of every experiment against the oracle, at test_gpu_sweep.py's bar."""
    _force(monkeypatch)
    monkeypatch.chdir(tmp_path)
    res = sweep.run_batch(P.G_TUPLES, seeds=list(P.G_SEEDS), device=0, save_png=False, verbose=False, **P.G_SHAPE)
    assert [r[0] for r in res] == P.G_TUPLES
    for p8, seed, (_, (coop, rep_mean)) in zip(P.G_TUPLES, P.G_SEEDS, res):
        got = read_datasets(str(tmp_path / sweep.get_folder_name(*p8) / "data" / "experiment_data.h5"))
        op = P.oracle_params(P.sweep_row(p8), P.G_SHAPE["L"], P.G_SHAPE["iterations"], p8[2], p8[6], p8[7])
        ds, fin = O.run(op, np.random.RandomState(seed), collect_snapshots=True)
        assert set(got) == set(ds), sorted(set(got) ^ set(ds))
        for k, w in ds.items():
            g, w = np.asarray(got[k]), np.asarray(w)
            assert g.shape == w.shape, (p8, k, g.shape, w.shape)
            if k in APPROX:
                np.testing.assert_allclose(g, w, equal_nan=True, err_msg=f"{p8} {k}", **FLOAT_TOL)
            else:
                assert np.array_equal(g, w, equal_nan=w.dtype.kind == "f"), (p8, k)
        assert coop == float(np.sum(fin["S"] == 0)) / fin["S"].size and rep_mean == 0


# ---- h. per-replica eps tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng", P.RNGS)
def test_per_replica_epsilon_tables(rng, monkeypatch):
    """Replicas identical but for (epsilon, epsilon_decay, epsilon_min), one seed: each follows its
    own schedule -- and no two schedules end in the same strategies, so a replica on another's
    table could not pass."""
    _force(monkeypatch)
    b = P.batch_h(rng)
    recs = P.records(b)
    eng = BatchEngine(b.L, b.T, _reps(b), use_second_order=b.M2, state_representation=b.state, rng=b.rng,
                      algorithm=b.alg)
    try:
        eng.run(snapshots=False)
        _check(eng, recs)
        hist = eng.histories()
        finals = [eng.final_state(k)[2] for k in range(len(recs))]
    finally:
        eng.close()
    for k, rec in enumerate(recs):
        m = rec.last - 1 if rec.stop_iter else rec.last
        assert np.array_equal(hist[k]["coop_rate_history"], rec.value[1:rec.last + 1, R.NCOOP] / rec.n), k
        assert np.array_equal(hist[k]["switch_C_to_D"], rec.value[1:m + 1, R.SW_CD]), k
        assert np.array_equal(hist[k]["switch_D_to_C"], rec.value[1:m + 1, R.SW_DC]), k
    for i in range(len(recs)):
        for j in range(i):
            assert not np.array_equal(finals[i], finals[j]), (i, j)
            assert not np.array_equal(recs[i].final["S"], recs[j].final["S"]), (i, j)
