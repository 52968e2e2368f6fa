"""The oracle's side of the learned policy record (spgg_policy): per replica and iteration t the
host model (spgg_amd.policy.host_policy_record) applied to the oracle's table, strategies and
get_state at the START of t -- the initial table for t = 1, else what on_step hands out after
iteration t-1 -- and, for the guards, the same on the table without iteration t-1's
neighbour-influence term (what the device's Q buffer holds between two step launches).
NumPy only; no GPU, no engine."""
import dataclasses
import functools

import numpy as np

from oracle import philox as PH
from oracle import spgg_oracle as O
from spgg_amd.policy import host_policy_record, policy_bin_edges
from tests import _params as P

BINS, GAP_RANGE = 8, 0.5        # the gaps of a dozen iterations lie within +-0.5 and beyond +-0.02


@dataclasses.dataclass
class Expected:
    rows: dict          # t -> the record row of iteration t (t = 1 .. last, and last + 1 for a replica still running)
    planes: dict        # t -> the plane
    bare: dict          # t -> the row on the table without iteration t-1's NI term (t >= 2)
    last: int           # iterations with a start record (the absorbing one included)
    stop_iter: int
    kappa: float
    params: O.Params
    final: dict


def _freeze(row):
    return tuple(sorted(row.items()))


@functools.lru_cache(maxsize=None)      # one oracle run per replica, shared by every test that needs it; read only
def _expected(rng, L, T, M2, state, alg, seed, stream_id, frozen, bins, gap_range):
    row = dict(frozen)
    p = P.oracle_params(row, L, T, M2, state, alg)
    edges = policy_bin_edges(gap_range, bins)
    rs = np.random.RandomState(seed)
    Q0, tables0 = O.init_tables(p, rs)          # as engine.reference_init draws them
    S0 = rs.randint(0, 2, size=(L, L))
    out = Expected({}, {}, {}, 0, 0, float(row["influence_factor"]), p, {})
    out.rows[1], out.planes[1] = host_policy_record(Q0, S0, O.get_state(S0, np.zeros((L, L)), p), bins, edges)
    ii, jj = np.indices((L, L))

    def on_step(i, S, R, Q, d):
        z = O.get_state(S, R, p)
        out.rows[i + 1], out.planes[i + 1] = host_policy_record(Q, S, z, bins, edges)
        bare = np.array(Q)
        bare[ii, jj, d["_old_states"], d["_actions"]] -= d["_nu"]
        out.bare[i + 1] = host_policy_record(bare, S, z, bins, edges)[0]

    draws = None
    if rng == "philox":
        key = PH.philox_key(int(seed or 0), stream_id)
        draws = lambda i: PH.draws(key, L, i, alg)   # noqa: E731
    _, fin = O.run(p, rs, S_init=S0, Q_init=Q0, tables_init=tables0, collect_snapshots=False, on_step=on_step,
                   draws=draws)
    out.stop_iter = int(fin["stop_iter"])
    out.last = out.stop_iter if out.stop_iter else T
    out.final = fin
    return out


def expected(b, bins=BINS, gap_range=GAP_RANGE):
    """[Expected] of the replicas of a tests/_params.Batch, as the engine runs them: replica k seeded
    b.seeds[k] and (Philox) drawing stream k."""
    return [_expected(b.rng, b.L, b.T, b.M2, b.state, b.alg, s, k if b.rng == "philox" else 0, _freeze(row), bins,
                      gap_range) for k, (row, s) in enumerate(zip(b.rows, b.seeds))]


def guards(exp, absorbing=False):
    """The oracle's side of a batch cannot be empty: every kappa != 0 replica has a recorded row the
    pending term changes the class counts of, kappa == 0 replicas have none, all four classes and
    both states occur, and (outside the absorption cases) at most one replica in eight absorbs early."""
    classes, states = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.int64)
    for k, e in enumerate(exp):
        moved = [t for t in range(2, e.last + 1) if not np.array_equal(e.rows[t][:16], e.bare[t][:16])]
        if e.kappa != 0.0 and e.last >= 2:
            assert moved, (k, "the pending term never changes a greedy policy")
        if e.kappa == 0.0:
            assert all(np.array_equal(e.rows[t], e.bare[t]) for t in range(2, e.last + 1)), k
        for t in range(1, e.last + 1):
            c = e.rows[t][:16].reshape(4, 2, 2)
            classes += c.sum(axis=(1, 2))
            states += c.sum(axis=(0, 1))
            n = e.params.L ** 2
            assert e.rows[t][:16].sum() == n and e.rows[t][16:21].sum() == 2 * n, (k, t)
    assert classes.all() and states.all(), (classes, states)
    if not absorbing:
        early = sum(1 for e in exp if e.stop_iter)
        assert 8 * early <= len(exp), early


def history_rows(e, every=1, t0=1):
    """The rows BatchEngine.policy_histories gives for the replica: t = t0, t0 + every, .. <= last."""
    its = np.arange(t0, e.last + 1, every, dtype=np.int64)
    return its, np.stack([e.rows[int(t)] for t in its])
