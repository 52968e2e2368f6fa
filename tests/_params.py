"""Seeded rows of the runner's parameter space, the named edge rows, the batches the parameter
tests run, and an exact model of the kernel's division.  NumPy + fractions; no GPU, no engine.

A row is a dict over tests/_record.PARAM_KEYS plus alg_alpha / alg_gamma, the operator's own
learning rate and discount (spgg_rep_params.alpha / gamma) where they differ from the model's
(diag_alpha / diag_gamma: the `algorithm_instance` case).  rows() draws every field of every row,
so the replicas of one batch differ in all of them; EDGE changes one field of R.BASE at a time.
tests/test_param_space_cpu.py holds the oracle's side of every batch (finite, few absorbed, both
strategies alive), tests/test_gpu_param_space.py the device's.
"""
import collections
import functools
import types
from fractions import Fraction

import numpy as np

from oracle import spgg_oracle as O
from tests import _record as R

ROW_KEYS = R.PARAM_KEYS + ("alg_alpha", "alg_gamma")
UNITS = (1.0, 0.5, 0.25, 2.0 ** -6, 2.0 ** -10)
ALGS = ("qlearning", "sarsa", "expected_sarsa", "double_qlearning")


def _dyadic(rs, i):
    """A reputation quadruple on the unit UNITS[i % 5]: integer multiples of it with every
    reachable R / unit in int8 (bounds within -128 .. 127; R moves by whole gains and losses and
    is clipped to the bounds, so it never leaves them)."""
    u = UNITS[i % len(UNITS)]
    k_gain, k_loss = int(rs.randint(1, 9)) | 1, int(rs.randint(1, 9))      # odd gain: no coarser unit fits
    k_min, k_max = int(rs.randint(8, 129)), int(rs.randint(8, 128))
    return dict(rep_gain_C=k_gain * u, delta_R_D=k_loss * u, R_min=-k_min * u, R_max=k_max * u)


def _free(rs):
    return dict(rep_gain_C=float(rs.uniform(0.1, 2)), delta_R_D=float(rs.uniform(0.1, 2)),
                R_min=-float(rs.uniform(1, 12)), R_max=float(rs.uniform(1, 12)))


def rows(seed, count, classes="mixed"):
    """`count` rows from RandomState(seed).  classes: "dyadic", "free", or "mixed" (odd rows free).
    Every fourth row (index 3, 7, ..) has influence_factor 0."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        row = dict(
            r=float(rs.uniform(0.5, 6)), c=float(rs.uniform(0.5, 2)), cost=float(rs.uniform(0, 2)),
            alpha=float(rs.uniform(0.05, 1)), gamma=float(rs.uniform(0, 1)),
            epsilon=float(rs.uniform(0.05, 1)), epsilon_decay=float(rs.uniform(0.9, 1)),
            epsilon_min=float(rs.uniform(0, 0.2)), lambda_epsilon=float(10.0 ** rs.uniform(-6, 0)),
            reward_weight_payoff=float(rs.uniform(0, 1)),
            alg_alpha=float(rs.uniform(0.05, 1)), alg_gamma=float(rs.uniform(0, 1)))
        kappa = float(rs.uniform(0.1, 3))
        row["influence_factor"] = 0.0 if i % 4 == 3 else kappa
        free = classes == "free" or (classes == "mixed" and i % 2 == 1)
        dy, fr = _dyadic(rs, i), _free(rs)          # both drawn: a row's other fields do not depend on its class
        row.update(fr if free else dy)
        assert set(row) == set(ROW_KEYS)
        assert (unit_of(row) is None) == free, row
        out.append(row)
    return out


def unit_of(row):
    """The dyadic reputation unit of a row (engine.ReplicaParams.rep_unit), or None."""
    return R._rep_unit(types.SimpleNamespace(**row))


def _edge(**kw):
    return dict(R.BASE, alg_alpha=None, alg_gamma=None, **kw)


# Each edge row is R.BASE with one change (two fields where one alone does not make the edge).
EDGE = {
    "w_p_0": _edge(reward_weight_payoff=0.0),
    "w_p_1": _edge(reward_weight_payoff=1.0),
    "alpha_0": _edge(alpha=0.0),
    "alpha_1": _edge(alpha=1.0),
    "gamma_0": _edge(gamma=0.0),
    "gamma_1": _edge(gamma=1.0),
    "always_explore": _edge(epsilon=1.0, epsilon_decay=1.0),
    "never_explore": _edge(epsilon=0.0, epsilon_min=0.0),
    "r_5": _edge(r=5.0),                    # norm_min = r - 5 = 0
    "r_6p5": _edge(r=6.5),
    "r_0p25": _edge(r=0.25),
    "cost_0": _edge(cost=0.0),
    "cost_4": _edge(cost=4.0),              # every payoff negative
    "c_0p7": _edge(c=0.7),
    "lambda_1e-12": _edge(lambda_epsilon=1e-12),
    "lambda_50": _edge(lambda_epsilon=50.0),
    "kappa_1e-9": _edge(influence_factor=1e-9),
    "kappa_25": _edge(influence_factor=25.0),
    "rep_gain_0": _edge(rep_gain_C=0.0),
    "rep_loss_0": _edge(delta_R_D=0.0),
    "rep_bounds_0": _edge(R_min=0.0, R_max=0.0),
    # bounds of +-128 units: R_max / unit is past int8, so this row (and a batch holding it) runs
    # the f64 reputation planes
    "rep_smallest_unit": _edge(rep_gain_C=2.0 ** -10, delta_R_D=3 * 2.0 ** -10, R_min=-0.125, R_max=0.125),
    "rep_int8_limits": _edge(rep_gain_C=1.0, delta_R_D=127.0, R_min=-128.0, R_max=127.0),
}
# The same rows (in place, so seeds and stream ids stay) as a batch the int8 reputation lattice runs:
# the smallest unit with its upper bound one unit lower (-128 .. 127 units).
EDGE_INT8 = {("rep_smallest_unit_int8" if k == "rep_smallest_unit" else k):
             (dict(v, R_max=127 * 2.0 ** -10) if k == "rep_smallest_unit" else v) for k, v in EDGE.items()}


# ---- row -> the two parameter types ----------------------------------------------------------------
def replica_params(row, seed):
    """engine.ReplicaParams of a row (imported here: this module stays importable without torch)."""
    from spgg_amd.engine import ReplicaParams
    return ReplicaParams(seed=seed, **{k: row[k] for k in ROW_KEYS})


def oracle_params(row, L, T, M2, state, algorithm):
    """oracle.Params of a row."""
    return R.oracle_params(row, L, T, M2, state, algorithm)


# ---- the batches of tests/test_gpu_param_space.py ---------------------------------------------------
# One batch = one engine: `rows` are its replicas in order, replica k seeded seeds[k] and (Philox)
# drawing stream k.
Batch = collections.namedtuple("Batch", "name rng L T M2 state alg rows seeds")

CONFIGS_B = [(False, "reputation"), (True, "action"), (True, "reputation")]
RNGS = ("mt19937", "philox")
B_ROWS = {"dyadic": rows(101, 12, "dyadic"), "mixed": rows(102, 12, "mixed")}
# the tile rows of tests/test_gpu_record.CTW_ROWS that have a compile-time width 20 (no Double-Q)
CTW_ROWS = [(False, "action", "qlearning", "dyadic"), (True, "reputation", "sarsa", "mixed"),
            (False, "reputation", "expected_sarsa", "mixed"), (True, "reputation", "qlearning", "dyadic")]
D_ROWS = {"dyadic": rows(103, 6, "dyadic"), "mixed": rows(104, 6, "mixed")}
E_ROWS = {7: rows(105, 7, "dyadic"), 11: rows(106, 11, "mixed")}
A_ROWS = rows(107, 48, "mixed")


def _seeds(base, n):
    return tuple(range(base, base + n))


def batch_b(kind, alg, M2, state, rng, L=18, T=40):
    return Batch(f"b-{kind}", rng, L, T, M2, state, alg, B_ROWS[kind], _seeds(200, 12))


def batch_c(kind, alg, rng):
    edge = EDGE if kind == "edge" else EDGE_INT8
    return Batch(f"c-{kind}", rng, 18, 40, True, "reputation", alg, list(edge.values()), _seeds(300, len(edge)))


def batch_d(L, M2, state, alg, kind):
    return Batch(f"d-{kind}", "philox", L, 12, M2, state, alg, D_ROWS[kind], _seeds(400, 6))


def batch_e(n):
    return Batch(f"e-{n}", "philox", 18, 40, True, "reputation", "qlearning", E_ROWS[n], _seeds(500, n))


def batch_f(L):
    """b's dyadic batch; L = 60 (T = 12) is the smallest lattice with a persistent launch."""
    return batch_b("dyadic", "qlearning", True, "reputation", "philox", L=L, T=40 if L == 18 else 12)


# g: eight sweep tuples (r, kappa, M2, alpha, w_P, gain, state, algorithm) sharing order, state and
# operator -- one BatchEngine in sweep.run_batch -- and differing in the other five fields
G_TUPLES = [(r, kappa, True, alpha, w_p, gain, "reputation", "qlearning") for r, kappa, alpha, w_p, gain in [
    (3.0, 1.0, 0.8, 0.95, 1.0), (3.6, 0.0, 0.5, 1.0, 0.5), (4.2, 0.5, 0.3, 0.8, 0.25), (2.5, 1.5, 0.9, 0.6, 2.0),
    (4.6, 0.0, 0.1, 0.95, 0.0), (3.3, 2.0, 0.65, 0.5, 1.0), (5.0, 0.25, 0.8, 0.7, 0.5), (1.5, 1.0, 0.2, 0.9, 1.5)]]
G_SEEDS = _seeds(600, 8)
G_SHAPE = dict(L=16, iterations=40)

# h: one row, six eps schedules (epsilon, epsilon_decay, epsilon_min), one seed: under MT19937 the
# replicas draw the same numbers and differ by their schedule alone
H_SCHEDULES = [(0.5, 0.99, 0.01), (0.5, 0.9, 0.05), (0.5, 0.99, 0.45), (0.9, 0.99, 0.01), (0.1, 1.0, 0.0),
               (1.0, 0.8, 0.15)]
H_ROWS = [dict(B_ROWS["dyadic"][0], epsilon=e, epsilon_decay=d, epsilon_min=m) for e, d, m in H_SCHEDULES]


def batch_h(rng):
    return Batch("h", rng, 18, 40, True, "reputation", "qlearning", H_ROWS, (700,) * len(H_ROWS))


def step_batches():
    """Every batch a GPU test steps and holds to the oracle's record."""
    out = [batch_b(kind, alg, M2, state, rng) for kind in B_ROWS for alg in ALGS for M2, state in CONFIGS_B
           for rng in RNGS]
    out += [batch_c(kind, alg, rng) for kind in ("edge", "int8") for alg in ("qlearning", "expected_sarsa")
            for rng in RNGS]
    out += [batch_d(L, M2, state, alg, kind) for L in (60, 120) for M2, state, alg, kind in CTW_ROWS]
    out += [batch_e(7), batch_e(11), batch_f(60)]
    out += [batch_h(rng) for rng in RNGS]
    return out


def all_rows():
    """name -> row of every distinct row the GPU tests use."""
    out = {}
    for kind, rs_ in B_ROWS.items():
        out.update({f"b-{kind}-{k}": r for k, r in enumerate(rs_)})
    out.update({f"edge-{k}": r for k, r in dict(EDGE, **EDGE_INT8).items()})
    for kind, rs_ in D_ROWS.items():
        out.update({f"d-{kind}-{k}": r for k, r in enumerate(rs_)})
    for n, rs_ in E_ROWS.items():
        out.update({f"e-{n}-{k}": r for k, r in enumerate(rs_)})
    out.update({f"a-{k}": r for k, r in enumerate(A_ROWS)})
    out.update({f"g-{k}": sweep_row(t) for k, t in enumerate(G_TUPLES)})
    out.update({f"h-{k}": r for k, r in enumerate(H_ROWS)})
    return out


# the sweep runner's model (sweep.RUNNER_MODEL, the reference's runner.py), restated: no engine import
RUNNER_MODEL = dict(c=1, cost=1, gamma=0.9, epsilon=0.5, epsilon_decay=0.99, epsilon_min=0.01, lambda_epsilon=0.01,
                    delta_R_D=1, R_min=-10, R_max=10)


def sweep_row(p8):
    r, kappa, _so, alpha, w_p, gain, _state, _alg = p8
    return dict(RUNNER_MODEL, r=r, influence_factor=kappa, alpha=alpha, reward_weight_payoff=w_p, rep_gain_C=gain,
                alg_alpha=None, alg_gamma=None)


def _freeze(row):
    return tuple((k, row[k]) for k in ROW_KEYS)


@functools.lru_cache(maxsize=None)      # one oracle run per replica, shared by every test that runs it; read only
def _record(rng, L, T, M2, state, alg, seed, stream_id, frozen):
    row = dict(frozen)
    if rng == "philox":
        return R.philox_record(L, T, row, seed, stream_id, M2, state, alg)
    return R.exact_record(row, L, T, M2, state, alg, rs=np.random.RandomState(seed))


def records(b):
    """The exact records (tests/_record.Record) of a batch's replicas."""
    return [_record(b.rng, b.L, b.T, b.M2, b.state, b.alg, s, k if b.rng == "philox" else 0, _freeze(row))
            for k, (row, s) in enumerate(zip(b.rows, b.seeds))]


# ---- a: payoff alone --------------------------------------------------------------------------------
A_SIDES = (5, 13, 24)


def payoff_strategies(L, count=48):
    """`count` initial strategy lattices (0 = C, 1 = D): Bernoulli lattices with defector densities
    from 0.05 to 0.95, then all-C, all-D, a checkerboard and stripes."""
    rs = np.random.RandomState(1000 + L)
    out = [(rs.rand(L, L) < d).astype(np.int64) for d in np.linspace(0.05, 0.95, count - 4)]
    i, j = np.indices((L, L))
    out += [np.zeros((L, L), dtype=np.int64), np.ones((L, L), dtype=np.int64), (i + j) % 2, (i // 2) % 2]
    return out


def table_reads(S):
    """{(table, N)} the payoff of lattice S reads: table 0 = pay_c (a cooperator's), 1 = pay_d, at
    the cooperator counts N of the agent's five groups."""
    N = O.sum5((S == 0).astype(int))
    seen = set()
    for g in [None, (1, 0), (-1, 0), (1, 1), (-1, 1)]:
        Ng = N if g is None else np.roll(N, *g)
        seen |= {(int(s), int(c)) for s, c in zip(S.ravel(), Ng.ravel())}
    return seen


# ---- the kernel's division ---------------------------------------------------------------------------
def div_uniform(x, d):
    """spgg_device.h's div_uniform(x, d, RN(1 / d)) in exact rational arithmetic: q = RN(x r),
    e = RN(x - q d) (one FMA), the result RN(q + e r) (one FMA).  float(Fraction) rounds to nearest
    even, as the hardware does."""
    X, D = Fraction(x), Fraction(d)
    r = float(1 / D)
    q = float(X * Fraction(r))
    e = float(X - Fraction(q) * D)
    return float(Fraction(q) + Fraction(e) * Fraction(r))


def payoff_quotients(row):
    """(x, d) of every payoff normalisation a row can make: x = tot - norm_min over the 2 * 6^5
    totals -- five table entries of one table, added in the kernel's (the reference's) order --
    and d = norm_den.  Returned without repeats."""
    rc = row["r"] * row["c"]
    tabs = [np.array([rc * N / 5 - row["cost"] for N in range(6)]), np.array([rc * N / 5 for N in range(6)])]
    norm_min = row["r"] - 5
    norm_den = 4 * row["r"] - norm_min
    xs = []
    for t in tabs:
        tot = t.copy()
        for _ in range(4):
            tot = (tot[..., None] + t).reshape(-1)      # ((((t0 + t1) + t2) + t3) + t4), every combination
        assert tot.size == 6 ** 5
        xs.append(tot - norm_min)
    return np.unique(np.concatenate(xs)), norm_den


def ni_quotients(row, L=18, steps=5, M2=True, seed=0):
    """[(x array, d)] of the neighbour-influence divisions of the first `steps` iterations of a
    row's oracle run: x = kappa * max(0, max_diff) per agent, d = gmax + lambda_epsilon."""
    out = []

    def on_step(i, S, Rn, Q, d):
        out.append((np.unique(row["influence_factor"] * np.maximum(0, d["_max_diff"])),
                    d["gmax"] + row["lambda_epsilon"]))

    O.run(oracle_params(row, L, steps, M2, "reputation", "qlearning"), np.random.RandomState(seed),
          collect_snapshots=False, on_step=on_step)
    return out
