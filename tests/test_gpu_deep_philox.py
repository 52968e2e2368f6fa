"""The Philox step kernels against the oracle through iteration 600 (tests/_deep.py).

bench.py times the step kernel on Philox draws at iterations 401-600; the other Philox tests
stop at t = 50.  Here every kernel family runs T = 600 -- across the turn boundary of
BatchEngine.run (256), across the eps floor (t = 390, where Expected SARSA's eps_{t-1} target
meets eps_t) and on the late lattice, where the reputation clip is the majority path, few agents
flip and most max_diff are 0 -- and every replica is held as tests/test_gpu_issue_cuts._run holds
its own: S, R, Q (Double-Q's two tables) and the stop iteration bit-equal to the oracle's, the
counters, the group composition and GMAX bit-equal on all 602 rows, the other slots under
tests/_record.bounds on the float rows of tests/_deep.ROWS.

a: the slot-word instance bench.py times (first order, Q-learning, compile-time width 40, four
agents per thread, one launch per iteration); b: it under Expected SARSA and SARSA; c: the
second order and Double-Q beside it at L = 120; d: the run-time-width kernels, every operator,
order and state at one and at the most agents per thread; e: replicas that absorb after the
first turn, at all-C and at all-D; f: persistent launches of up to 256 iterations, against the
oracle and against one launch per iteration.  tests/test_deep_philox_cpu.py holds the oracle's
side of every case; each case prints its oracle seconds and its device seconds.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from spgg_amd.engine import BatchEngine  # noqa: E402
from tests import _deep as D  # noqa: E402
from tests import _record as R  # noqa: E402
from tests import test_gpu_issue_cuts as C  # noqa: E402  (its helpers)
from tests._philox import check_final  # noqa: E402
from tests.test_gpu_record import STEP_SLOTS  # noqa: E402


def _ids(batches):
    return [b.name for b in batches]


def _hold(eng, recs):
    """A finished engine against the sparse records of its replicas; the folded record array."""
    assert eng.L in R.GPU_LATTICES      # (test_record_bounds_cpu.py holds the bounds at these lattices)
    st = eng.stats_folded().cpu().numpy()
    eng.all_stopped()
    assert st.shape == (len(recs), D.T + 2, R.NSTAT)
    for k, rec in enumerate(recs):
        bad = R.mismatches_on_rows(st[k], rec, R.bounds(rec, apt_max=4, rep_int8=eng.rep_int8))
        assert not bad, "replica %d: (t, slot, got, want, bound) %s (%d in all)" % (k, bad[:12], len(bad))
        assert int(eng.stopped[k]) == rec.stop_iter, (k, int(eng.stopped[k]), rec.stop_iter)
        check_final(eng.final_state(k), rec.final, k)
        if eng.double_q:
            q1, q2 = eng.final_tables(k)
            assert np.array_equal(q1, rec.final["tables"][0]) and np.array_equal(q2, rec.final["tables"][1]), k
    return st


def _go(b, monkeypatch, look, chunk=None, **env):
    """Run batch b to its end under `env` alone and hold it to the oracle; what the callers look at."""
    t0 = time.perf_counter()
    recs = D.records(b)
    t_oracle = time.perf_counter() - t0
    C._force(monkeypatch, **env)
    t0 = time.perf_counter()
    eng = BatchEngine(b.L, b.T, D.reps(b), use_second_order=b.M2, state_representation=b.state, rng=b.rng,
                      algorithm=b.alg)
    try:
        look(eng)
        assert eng.rep_int8         # the bench's int8 reputation path
        eng.run(snapshots=False, **({} if chunk is None else dict(chunk=chunk)))
        st = _hold(eng, recs)
        out = dict(st=st, recs=recs, final=[eng.final_state(k) for k in range(len(recs))],
                   stop=eng.stop_iter.cpu().numpy().copy())
        if b.alg == "expected_sarsa":
            for k, (rec, h) in enumerate(zip(recs, eng.histories())):
                want = D.epsilon_history(rec)
                got = np.asarray(h["epsilon_history_final"])
                assert got.dtype == want.dtype and np.array_equal(got, want), (k, "epsilon_history_final")
                if not rec.stop_iter:      # eps_{t-1} > eps_t = eps_min on the crossing iteration, equal after it
                    assert got[D.T_FLOOR - 2] > got[D.T_FLOOR - 1] == got[-1] == rec.params.epsilon_min
    finally:
        eng.close()
    print("seconds", b.name, env, "tile", eng.tile, "oracle %.2f" % t_oracle,
          "device and checks %.2f" % (time.perf_counter() - t0))
    return out


def _slot_word(eng):
    assert eng.tile == (40, 24), eng.tile
    assert C._compile_time_width_40(eng) and not eng.persistent


@pytest.mark.parametrize("b", D.A, ids=_ids(D.A))
def test_slot_word_instance(b, monkeypatch):
    _go(b, monkeypatch, _slot_word, SPGG_APT="max")


@pytest.mark.parametrize("b", D.B, ids=_ids(D.B))
def test_slot_word_instance_other_operators(b, monkeypatch):
    _go(b, monkeypatch, _slot_word, SPGG_APT="max")


@pytest.mark.parametrize("b", D.C, ids=_ids(D.C))
def test_beside_the_slot_word_instance(b, monkeypatch):
    def look(eng):
        if b.alg == "double_qlearning":      # tiles of <= 512 agents: a run-time width
            assert eng.tile[0] * eng.tile[1] <= 512 and not C._compile_time_width_40(eng), eng.tile
        else:
            assert b.M2 and eng.tile == (40, 24), eng.tile

    _go(b, monkeypatch, look, SPGG_APT="max")


@pytest.mark.parametrize("apt", ["1", "max"])
@pytest.mark.parametrize("b", D.D, ids=_ids(D.D))
def test_run_time_width_kernels(b, apt, monkeypatch):
    def look(eng):
        area = eng.tile[0] * eng.tile[1]
        if apt == "1":
            assert area <= 256, eng.tile
        elif b.alg == "double_qlearning":    # its most is two agents per thread (tiles of <= 512 agents)
            assert 256 < area <= 512, eng.tile
        else:
            assert area > 512, eng.tile
        assert not C._compile_time_width_40(eng) and eng.tile[0] != 20

    _go(b, monkeypatch, look, SPGG_APT=apt)


@pytest.mark.parametrize("b", D.E, ids=_ids(D.E))
def test_late_absorption(b, monkeypatch):
    """Replicas that absorb after the first turn of run(), beside ones that run to T: the final
    state is the state at the stop iteration (the oracle's, which stops there), the absorbing
    iteration records its start only, and every later row of the record is zero."""
    out = _go(b, monkeypatch, lambda eng: None)
    stops = D.e_stops(b)
    n = b.L * b.L
    for k, rec in enumerate(out["recs"]):
        st = out["st"][k]
        if k in stops:
            last = stops[k][0]
            assert rec.stop_iter == last == int(out["stop"][k]) and D.CHUNK < last < D.T
            assert st[last, R.NCOOP] == stops[k][1] and stops[k][1] in (0, n)
            assert st[last, R.SUMP] != 0.0 and st[last - 1, R.SUMQ:R.SUMQ + 4].all(), k
            assert not st[last, list(STEP_SLOTS)].any(), (k, "the absorbing iteration records its start only")
            assert not st[last + 1:].any(), (k, "rows past the last iteration")
        else:
            assert rec.stop_iter == 0 == int(out["stop"][k]) and st[D.T, R.SUMQ:R.SUMQ + 4].all(), k


@pytest.mark.parametrize("b", D.F, ids=_ids(D.F))
def test_persistent_launches(b, monkeypatch):
    """run(chunk=256): launches that carry 256, 256 and 88 iterations in registers; then the same
    replicas at one launch per iteration: S, R, Q and the stops identical."""
    def persistent(eng):
        assert eng.persistent and eng.tile[0] == 20, (eng.persist_capacity, eng.tile)

    def per_launch(eng):
        assert not eng.persistent and eng.tile[0] == 20, eng.tile

    a = _go(b, monkeypatch, persistent, chunk=D.CHUNK, SPGG_PERSIST="1", SPGG_APT="2")
    c = _go(b, monkeypatch, per_launch, chunk=D.CHUNK, SPGG_PERSIST="0", SPGG_APT="2")
    assert np.array_equal(a["stop"], c["stop"])
    for k, (x, y) in enumerate(zip(a["final"], c["final"])):
        for u, v in zip(x, y):
            assert np.array_equal(u, v), k
