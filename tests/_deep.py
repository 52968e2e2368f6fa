"""The deep Philox cases: T = 600, every step-kernel family held to the oracle past the turn
boundary of BatchEngine.run (256), the eps floor (t = 390 under R.BASE) and the late lattice,
where most reputations sit at a bound and few strategies flip.  NumPy only; no GPU, no engine.

tests/test_deep_philox_cpu.py holds the oracle's side (the cases are what they claim),
tests/test_gpu_deep_philox.py the device's.  One batch = one engine (tests/_params.Batch):
replica k is seeded seeds[k] and draws Philox stream k.  Every expectation is an oracle run made
at test time, once per replica (lru_cache), shared by both files and read only.

An exact record costs math.fsum on every float slot of every row; over 600 rows that is four
times the oracle run itself, so the records here evaluate the float slots on ROWS alone
(tests/_record.exact_record, `rows`): the start, the turn boundary, the floor crossing, the end
and every 50th iteration.  The counters, the group composition and GMAX are on every row.
"""
import functools

import numpy as np

from oracle import spgg_oracle as O
from tests import _params as P
from tests import _record as R

T = 600
ROWS = frozenset({1, 2, 3, 255, 256, 257, 258, 388, 389, 390, 391, 392, 598, 599, 600} | set(range(50, T + 1, 50)))
# eps_t, the value iteration t leaves (epsilon_history_final[t - 1]; the select of t + 1 draws against it),
# is epsilon_min from this t on under R.BASE (test_deep_philox_cpu.py)
T_FLOOR = 390
CHUNK = 256         # BatchEngine.run's turn


def _row(**kw):
    return dict(R.BASE, alg_alpha=None, alg_gamma=None, **kw)


def _one(name, L, M2, alg, seed, **kw):
    return P.Batch(name, "philox", L, T, M2, "reputation", alg, [_row(**kw)], (seed,))


# ---- a. the slot-word instance: first order, Q-learning, compile-time width 40, four agents per thread
KAPPA_WP_A = [(0.0, 1.0), (0.5, 1.0), (1.0, 1.0), (0.5, 0.95)]
A = [_one(f"a-kappa{k}-wp{w}", 120, False, "qlearning", 810 + i, r=3.5, influence_factor=k, reward_weight_payoff=w)
     for i, (k, w) in enumerate(KAPPA_WP_A)]
# ---- b. the same instance under the other operators
B = [_one(f"b-{alg}", 120, False, alg, 820 + i, r=3.5, influence_factor=0.5, reward_weight_payoff=1.0)
     for i, alg in enumerate(["expected_sarsa", "sarsa"])]
# ---- c. beside it at L = 120: the second order (compile-time width, (row, column) word) and
# Double-Q (tiles of <= 512 agents: a run-time width)
C = [_one("c-second_order", 120, True, "qlearning", 830, r=3.5, influence_factor=0.5, reward_weight_payoff=1.0),
     _one("c-double_qlearning", 120, False, "double_qlearning", 831, r=3.5, influence_factor=0.5,
          reward_weight_payoff=0.95)]

# ---- d. run-time-width kernels: every operator, order and state, one and the most agents per thread
REPS_D = [(2.5, 0.0, 11), (3.0, 1.0, 12), (4.2, 0.5, 13), (3.6, 1.5, 14)]       # (r, kappa, seed)


def _batch_d(name, L, alg, M2, state):
    return P.Batch(name, "philox", L, T, M2, state, alg, [_row(r=r, influence_factor=k) for r, k, _ in REPS_D],
                   tuple(s for _, _, s in REPS_D))


D = [_batch_d(f"d-{alg}-{'M2' if M2 else 'M1'}-{state}", 30, alg, M2, state)
     for alg in P.ALGS for M2, state in P.CONFIGS_B]

# ---- e. late absorption: d's replicas at L = 18.  (algorithm, M2, state) -> {replica: (stop iteration,
# cooperators at the stop)}; the other replicas of a batch run to T (test_deep_philox_cpu.py)
E_STOPS = {
    ("qlearning", True, "reputation"): {2: (332, 324)},
    ("sarsa", True, "reputation"): {2: (324, 324), 3: (594, 324)},
    ("expected_sarsa", True, "reputation"): {2: (441, 324), 3: (552, 324)},
    ("sarsa", False, "reputation"): {1: (591, 0)},
}
E = [_batch_d(f"e-{alg}-{'M2' if M2 else 'M1'}-{state}", 18, alg, M2, state) for alg, M2, state in E_STOPS]
# the float rows of e: ROWS and the rows around each stop (the absorbing iteration records its start only)
E_ROWS = frozenset(ROWS | {s + o for stops in E_STOPS.values() for s, _ in stops.values() for o in (-1, 0, 1)})

# ---- f. persistent launches at the smallest lattice that has one
F = [P.Batch("f-persistent", "philox", 60, T, False, "reputation", "qlearning",
             [_row(influence_factor=0.0), _row(influence_factor=1.0)], (840, 841))]

GROUPS = dict(a=A, b=B, c=C, d=D, e=E, f=F)


def e_stops(b):
    return E_STOPS[(b.alg, b.M2, b.state)]


def rows_of(b):
    return E_ROWS if b.name.startswith("e-") else ROWS


def reps(b):
    """engine.ReplicaParams of a batch's replicas."""
    return [P.replica_params(row, s) for row, s in zip(b.rows, b.seeds)]


@functools.lru_cache(maxsize=None)
def _record(L, M2, state, alg, seed, stream_id, frozen, rows, T_=T):
    return R.philox_record(L, T_, dict(frozen), seed, stream_id, M2, state, alg, rows=rows)


def records(b):
    """The sparse exact records of a batch's replicas (float slots on rows_of(b))."""
    return [_record(b.L, b.M2, b.state, b.alg, s, k, P._freeze(row), rows_of(b))
            for k, (row, s) in enumerate(zip(b.rows, b.seeds))]


def epsilon_history(rec):
    """The oracle's epsilon_history_final of a record's run: eps after each executed iteration."""
    m = rec.last - 1 if rec.stop_iter else rec.last
    return O.epsilon_schedule(rec.params, m + 1)[1:]


def share_at_bound(Rep, p):
    """Share of agents whose reputation sits at R_min or R_max: the clip was taken."""
    return float(np.mean((Rep == p.R_min) | (Rep == p.R_max)))


def reputation_after(b, k, t):
    """R after iteration t of replica k of batch b: a run of t iterations (a Philox draw depends on
    the iteration, not on the run's length), or the record's own final state at t = T."""
    if t == T:
        return records(b)[k].final["R"]
    return _record(b.L, b.M2, b.state, b.alg, b.seeds[k], k, P._freeze(b.rows[k]), (), t).final["R"]
