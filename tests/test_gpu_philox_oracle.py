"""The bench's random stream (rng="philox") against the oracle, bit for bit.

The Philox stream is a pure function of (seed, stream id, agent, iteration, select)
(include/spgg_abi.h, SPGG_RNG_PHILOX), modelled in NumPy by oracle/philox.py from the generator's
definition; the oracle takes those draws in place of RandomState's.  Every replica of every case
is held to the MT19937 tests' bar: S, R, Q (Double-Q: both tables), the stop iteration and the
integer histories bit-exact, float histories within 1e-5 (tests/_philox.check_replica).

Shapes are the smallest that reach each path: the run-time-width kernels at one and at four
agents per thread, an odd lattice (agent pairs straddle rows), the compile-time-width kernels
and their paired Philox blocks at widths 20 and 40 (the 40 x 24 tile of L = 120 has 64 invalid
slots), four agents per thread below the compile-time-width threshold, the key fold (high seed half, stream ids
off zero), and the eps = 1 .. 0 threshold edges with an absorbing replica."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from spgg_amd.engine import BatchEngine, ReplicaParams, reference_init  # noqa: E402
from tests._philox import EDGE_CASE, check_replica, philox_oracle  # noqa: E402

ALGS = ["qlearning", "sarsa", "expected_sarsa", "double_qlearning"]
ORDER_STATE = [(False, "reputation"), (True, "action"), (True, "reputation")]


def _runner_params(**kw):
    base = dict(c=1, cost=1, alpha=0.8, gamma=0.9, epsilon=0.5, epsilon_decay=0.99,
                epsilon_min=0.01, lambda_epsilon=0.01, delta_R_D=1, R_min=-10, R_max=10,
                rep_gain_C=1.0, reward_weight_payoff=0.95, influence_factor=1.0, r=3.0)
    base.update(kw)
    return ReplicaParams(**base)


def _force_apt(monkeypatch, apt):
    if apt is None:
        monkeypatch.delenv("SPGG_APT", raising=False)
    else:
        monkeypatch.setenv("SPGG_APT", apt)


def _run_and_check(L, T, reps, M2, state, alg, want, tile=None, **engine_kw):
    """Run the batch in Philox mode and hold every replica to its oracle run want[k] = (ds, fin)."""
    eng = BatchEngine(L, T, reps, use_second_order=M2, state_representation=state, rng="philox",
                      algorithm=alg, **engine_kw)
    try:
        if tile is not None:
            tile(eng)
        eng.run(snapshots=False)
        hs = eng.histories()
        for k in range(len(reps)):
            check_replica(eng, hs[k], k, *want[k])
        return [eng.final_state(k)[2] for k in range(len(reps))]
    finally:
        eng.close()


# ---- a. run-time-width kernels: every operator, order, state; one and four agents per thread ----
REPS_A = [(2.5, 0.0, 11), (3.0, 1.0, 12), (4.2, 0.5, 13), (1.0, 1.5, 14)]


def _reps_a():
    return [_runner_params(r=r, influence_factor=k, seed=s) for r, k, s in REPS_A]


@functools.lru_cache(maxsize=None)      # one oracle run per configuration, shared by both tilings; read only
def _want_a(alg, M2, state):
    return [philox_oracle(18, 50, p, k, M2, state, alg) for k, p in enumerate(_reps_a())]


@pytest.mark.parametrize("apt", ["1", "max"])
@pytest.mark.parametrize("alg", ALGS)
@pytest.mark.parametrize("M2,state", ORDER_STATE)
def test_operators_match_philox_oracle(alg, M2, state, apt, monkeypatch):
    _force_apt(monkeypatch, apt)
    _run_and_check(18, 50, _reps_a(), M2, state, alg, _want_a(alg, M2, state))


# ---- b. odd lattice: agent pairs (2m, 2m+1) straddle rows ----
@pytest.mark.parametrize("alg", ALGS)
def test_odd_lattice_matches_philox_oracle(alg, monkeypatch):
    _force_apt(monkeypatch, None)
    L, T = 13, 40
    reps = [_runner_params(r=r, seed=s) for r, s in [(3.0, 31), (4.0, 32)]]
    want = [philox_oracle(L, T, p, k, True, "reputation", alg) for k, p in enumerate(reps)]

    def tile(eng):      # the one-agent-per-thread kernels
        assert eng.tile[0] * eng.tile[1] <= 256, eng.tile

    _run_and_check(L, T, reps, True, "reputation", alg, want, tile)


# ---- c. compile-time width (20, 40) and the paired Philox blocks, at their smallest sides ----
CTW_ROWS = [
    (False, "action", "qlearning", 1.0),
    (True, "reputation", "sarsa", 0.3),            # non-dyadic gain: f64 reputation planes
    (False, "reputation", "expected_sarsa", 0.3),
    (True, "action", "double_qlearning", 1.0),
    (False, "reputation", "double_qlearning", 0.3),
    (True, "reputation", "qlearning", 1.0),
]


def _ctw(L, apt, M2, state, alg, gain, monkeypatch, want_tile):
    _force_apt(monkeypatch, apt)
    T = 40
    reps = [_runner_params(seed=s, rep_gain_C=gain, r=3.0 + 0.4 * s) for s in (5, 6)]
    want = [philox_oracle(L, T, p, k, M2, state, alg) for k, p in enumerate(reps)]
    _run_and_check(L, T, reps, M2, state, alg, want, want_tile)


@pytest.mark.parametrize("M2,state,alg,gain", [r for r in CTW_ROWS if r[2] != "double_qlearning"])
def test_width_20_tiles_match_philox_oracle(M2, state, alg, gain, monkeypatch):
    """L = 60, two agents per thread (Double-Q has no compile-time width 20)."""
    def tile(eng):
        assert eng.tile[0] == 20, eng.tile

    _ctw(60, "2", M2, state, alg, gain, monkeypatch, tile)


@pytest.mark.parametrize("M2,state,alg,gain", CTW_ROWS)
def test_width_40_tiles_match_philox_oracle(M2, state, alg, gain, monkeypatch):
    """L = 120, four agents per thread: 40 x 24 tiles, 960 of a workgroup's 1024 slots valid."""
    def tile(eng):
        if alg != "double_qlearning":       # Double-Q tiles hold <= 512 agents: run-time width
            assert eng.tile == (40, 24), eng.tile

    _ctw(120, "max", M2, state, alg, gain, monkeypatch, tile)


# ---- d. four agents per thread below the compile-time-width threshold (L < 120): run-time width ----
@pytest.mark.parametrize("M2", [False, True])
def test_four_agents_per_thread_run_time_width_matches_philox_oracle(M2, monkeypatch):
    """L = 80: the chooser's 27 x 27 tiles (729 agents: four per thread), which do not divide L --
    the last tile row and column hold cells outside the lattice."""
    _force_apt(monkeypatch, "max")
    L, T = 80, 30
    reps = [_runner_params(r=r, seed=s) for r, s in [(3.0, 41), (4.4, 42)]]
    want = [philox_oracle(L, T, p, k, M2, "reputation") for k, p in enumerate(reps)]

    def tile(eng):
        assert 512 < eng.tile[0] * eng.tile[1] <= 1024 and L < 120, eng.tile

    _run_and_check(L, T, reps, M2, "reputation", "qlearning", want, tile)


# ---- e. the key: both seed halves and stream ids off zero ----
def test_key_uses_both_seed_halves_and_the_stream_id(monkeypatch):
    _force_apt(monkeypatch, None)
    L, T, off = 16, 20, 3
    big = 0x9E3779B97F4A7C15
    reps = [_runner_params(seed=s) for s in (big, big, big & 0xFFFFFFFF)]
    init = reference_init(L, np.random.RandomState(7))     # RandomState takes no seed >= 2^32
    want = [philox_oracle(L, T, p, off + k, False, "reputation", init=init) for k, p in enumerate(reps)]
    S = _run_and_check(L, T, reps, False, "reputation", "qlearning", want, init=[init] * 3, replica_offset=off)
    assert not np.array_equal(S[0], S[1])       # one seed, stream ids 3 and 4
    assert not np.array_equal(S[0], S[2]) and not np.array_equal(S[1], S[2])


# ---- f. eps edges (1, then halved towards 0) and absorption ----
def test_epsilon_edges_and_absorption_match_philox_oracle(monkeypatch):
    _force_apt(monkeypatch, None)
    L, T = EDGE_CASE["L"], EDGE_CASE["T"]
    reps = [ReplicaParams(**kw) for kw in EDGE_CASE["replicas"]]
    assert all(p.epsilon == 1.0 and p.epsilon_decay == 0.5 and p.epsilon_min == 0.0 for p in reps)
    want = [philox_oracle(L, T, p, k, False, "reputation") for k, p in enumerate(reps)]
    stops = [fin["stop_iter"] for _, fin in want]
    assert any(0 < s < T for s in stops), stops     # (test_philox_oracle_cpu.py keeps this true)
    eng = BatchEngine(L, T, reps, use_second_order=False, rng="philox")
    try:
        eng.run(snapshots=False)
        hs = eng.histories()
        for k, (ds, fin) in enumerate(want):
            assert int(eng.stopped[k]) == fin["stop_iter"], (k, eng.stopped[k], fin["stop_iter"])
            for key in ("coop_rate_history", "epsilon_history_final", "switch_C_to_D", "rep_avg_history_final"):
                assert len(hs[k][key]) == len(ds[key]), (k, key)
            check_replica(eng, hs[k], k, ds, fin)
    finally:
        eng.close()
