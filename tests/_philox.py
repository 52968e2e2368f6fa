"""The oracle run in the device's Philox stream (oracle/philox.py), and the per-replica bar the
Philox tests hold the engine to: S, R, Q, stop iteration, counts and integer histories bit for
bit, float histories within the project's 1e-5.  NumPy only (spawned oracle workers import it)."""
import numpy as np

from oracle import philox as PH
from oracle import spgg_oracle as O

FLOAT_TOL = dict(rtol=1e-5, atol=1e-9)
EXACT_KEYS = ("coop_rate_history", "switch_C_to_D", "switch_D_to_C", "epsilon_history_final") + tuple(
    f"group_comp_d{d}_history" for d in range(6))
# the float histories of test_gpu_cfg3.py and test_gpu_cfg4.py
FLOAT_KEYS = ("neighbor_influence_percent", "best_neighbor_second_order_percent", "rep_avg_history_final",
              "it_records_final", "avg_reward_C_history", "avg_reward_D_history", "payoff_component_history",
              "rep_component_history", "avg_q_s0_c_history", "avg_q_s1_d_history", "cooperators_q_s0_c_history",
              "cooperators_q_s0_d_history", "defectors_q_s1_c_history", "defectors_q_s1_d_history")
PARAM_KEYS = ("r", "c", "cost", "alpha", "gamma", "epsilon", "epsilon_decay", "epsilon_min", "influence_factor",
              "lambda_epsilon", "delta_R_D", "R_min", "R_max", "reward_weight_payoff", "rep_gain_C")

# The eps-edge / absorption case of test_gpu_philox_oracle.py: eps = 1 (every agent explores), then
# 2^-1, 2^-2, .. down through the 31-bit threshold's last steps (2^-31 and below: thr31 = 1) towards
# 0; replica k draws stream k.  test_philox_oracle_cpu.py checks that one of them absorbs before T.
_EDGE_BASE = dict(c=1, cost=1, alpha=0.8, gamma=0.9, epsilon=1.0, epsilon_decay=0.5, epsilon_min=0.0,
                  influence_factor=1.0, lambda_epsilon=0.01, delta_R_D=1, R_min=-10, R_max=10,
                  reward_weight_payoff=0.95, rep_gain_C=1.0)
EDGE_CASE = dict(L=16, T=80, replicas=[dict(_EDGE_BASE, r=0.5, seed=21), dict(_EDGE_BASE, r=3.0, seed=22)])


def param_dict(p):
    """The oracle's keyword arguments of a ReplicaParams (plain floats: picklable)."""
    return {k: getattr(p, k) for k in PARAM_KEYS}


def philox_oracle_kw(L, T, kw, seed, stream_id, M2, state, algorithm="qlearning", init=None):
    """(datasets, final) of the oracle under the Philox draws of (seed, stream_id).

    init: an object with Q, S and (Double-Q) tables; None: SPGG.__init__'s draws from
    RandomState(seed), as the engine initialises a replica (engine.reference_init)."""
    op = O.Params(L=L, iterations=T, use_second_order=M2, state_representation=state, algorithm=algorithm, **kw)
    if init is None:
        rs = np.random.RandomState(seed)
        Q, tables = O.init_tables(op, rs)
        S = rs.randint(0, 2, size=(L, L))
    else:
        Q, tables, S = init.Q, init.tables, init.S
    key = PH.philox_key(int(seed or 0), stream_id)
    return O.run(op, None, S_init=S, Q_init=Q, tables_init=tables, collect_snapshots=False,
                 draws=lambda i: PH.draws(key, L, i, algorithm))


def philox_oracle(L, T, p, stream_id, M2, state, algorithm="qlearning", init=None):
    """philox_oracle_kw for a ReplicaParams p (seed p.seed); stream_id = replica_offset + k."""
    return philox_oracle_kw(L, T, param_dict(p), p.seed, stream_id, M2, state, algorithm, init)


def philox_oracle_job(job):
    """philox_oracle_kw(*job) for a spawned worker; final cut down to what the checks read."""
    ds, fin = philox_oracle_kw(*job)
    return ds, {k: fin[k] for k in ("S", "R", "Q", "tables", "stop_iter")}


def check_final(got, fin, what):
    """got = (Q, R, S) of BatchEngine.final_state (or of a dump) against the oracle's final."""
    Q, R, S = got
    assert np.array_equal(S, fin["S"]), (what, "S", int(np.sum(S != fin["S"])))
    assert np.array_equal(R, fin["R"]), (what, "R")
    assert np.array_equal(Q, fin["Q"]), (what, "Q")


def check_replica(eng, hist, k, ds, fin, what=None):
    """Replica k of a finished engine run (hist = eng.histories()[k]) against the oracle's (ds, fin)."""
    what = k if what is None else what
    check_final(eng.final_state(k), fin, what)
    if eng.double_q:
        q1, q2 = eng.final_tables(k)
        assert np.array_equal(q1, fin["tables"][0]) and np.array_equal(q2, fin["tables"][1]), (what, "tables")
    assert int(eng.stopped[k]) == int(fin["stop_iter"]), (what, int(eng.stopped[k]), fin["stop_iter"])
    for key in EXACT_KEYS:
        assert hist[key].shape == ds[key].shape, (what, key, hist[key].shape, ds[key].shape)
        assert np.array_equal(hist[key], ds[key]), (what, key)
    for key in FLOAT_KEYS:
        assert hist[key].shape == ds[key].shape, (what, key, hist[key].shape, ds[key].shape)
        np.testing.assert_allclose(hist[key], ds[key], equal_nan=True, err_msg=f"{what} {key}", **FLOAT_TOL)
