"""Drop-in `SPGG` (src/model/spgg.py:39-637) whose run loop executes on the MI355X.

Same constructor signature, attributes, random-stream consumption, datasets
and return value as the reference, so `src/experiments/runner.py:88-105` can
construct and run it unchanged.  Construction stays on the host (it is the
reference's own one-off NumPy init: entropy reseed, Q ~ U(-0.01,0.01),
random population).  `run()` hands the continuing global MT19937 key to the
device, which reproduces every step of spgg.py:368-592 bit for bit in
libspgg_hip.so, then writes the reference's dataset layout.
"""
from __future__ import annotations

import os

import numpy as np

from . import algorithms as A
from .dwell import DWELL_DATASETS, DWELL_FIELD_DATASETS
from .engine import BatchEngine, InitState, ReplicaParams, SNAPSHOT_ITERS
from .h5io import open_writer
from .pairmap import PAIR_MAP_DISTANCE_DATASET, PAIR_MAP_ITERS_DATASET, field_pairs
from .payoff import PAYOFF_DATASETS, PAYOFF_MAP_DATASET, PAYOFF_PAIRS_DATASET
from .policy import POLICY_DATASETS, POLICY_MAP_DATASET


def _sum5(A_):
    return A_ + np.roll(A_, -1, axis=0) + np.roll(A_, 1, axis=0) + np.roll(A_, -1, axis=1) + np.roll(A_, 1, axis=1)


def sum_position_and_neighbors(A_):
    """5-point periodic sum (spgg.py:23-36); host utility kept for API parity."""
    return _sum5(A_)


def _count(v):
    return int(v or 0)


# The in-run record options: class attributes of SPGG (not constructor arguments; the sweep takes
# them among its model overrides), name -> (default, BatchEngine.run keyword argument, conversion).
# *_every = k > 0: also record S_t (and R_t) at t = 1, 1+k, ... on the device and write the record as
# more datasets after the reference's own; 0: the reference's file.
RECORD_OPTIONS = {
    # the cooperator clusters (count, largest, C-D bonds: CLUSTER_DATASETS); _periodic: they wrap
    # with the lattice (the final cluster_sizes dataset never does: spgg.py:631)
    "cluster_history_every": (0, "clusters_every", _count),
    "cluster_history_periodic": (False, "clusters_periodic", bool),
    # the cooperator pair counts along rows and columns at the distances 0 .. correlation_max_distance
    # (None: L // 2; CORRELATION_DATASETS)
    "correlation_history_every": (0, "correlations_every", _count),
    "correlation_max_distance": (None, "correlations_max_d", lambda v: v),
    # the joint histogram strategy x reputation bin (reputation_history_bins bins over R_min .. R_max)
    # and, with reputation_max_distance not None, the pair sums of the int8 reputation plane at the
    # distances 0 .. reputation_max_distance (REPUTATION_DATASETS)
    "reputation_history_every": (0, "reputation_every", _count),
    "reputation_history_bins": (20, "reputation_bins", int),
    "reputation_max_distance": (None, "reputation_max_d", lambda v: v),
}


# The strategy dwell record's options (dwell.py), class attributes of SPGG like the RECORD_OPTIONS but
# a table of their own: the record is not one of records.KINDS.  name -> (default, conversion).
# dwell_history_every = k > 0: track every agent's strategy changes from iteration 1 on and write the
# DWELL_DATASETS (rows at t = 1, 1+k, ...) after the other records' datasets; dwell_fields: also the
# per-agent DWELL_FIELD_DATASETS of the final state.
DWELL_OPTIONS = {
    "dwell_history_every": (0, _count),
    "dwell_fields": (False, bool),
}


# The learned policy record's options (policy.py), class attributes of SPGG in a table of their own as
# the dwell record's are.  name -> (default, conversion).  policy_history_every = k > 0: record the
# policy field (classes by strategy and state, bonds, gap histograms) at t = 1, 1+k, ... on the device
# and write the POLICY_DATASETS after the dwell datasets; _bins and _gap_range (a number g for (-g, g),
# or a (lo, hi) pair): the gap histogram; policy_map_final: also the final state's per-agent map
# class | strategy << 2 | state << 3 (uint8) as POLICY_MAP_DATASET.
POLICY_OPTIONS = {
    "policy_history_every": (0, _count),
    "policy_history_bins": (32, int),
    "policy_history_gap_range": (2.0, lambda v: v),
    "policy_map_final": (False, bool),
}


# The payoff record's options (payoff.py), class attributes of SPGG in a table of their own as the policy
# record's are.  name -> (default, conversion).  payoff_history_every = k > 0: record the payoff field
# (the census of strategy x cooperating neighbours x group-cooperator total, and the bonds by their
# difference in that total) at t = 1, 1+k, ... on the device and write the PAYOFF_DATASETS after the
# policy datasets; payoff_max_distance not None: also the pair sums of K and c at the distances
# 0 .. payoff_max_distance (PAYOFF_PAIRS_DATASET); payoff_map_final: also the final state's per-agent
# map K | strategy << 5 | (m & 3) << 6 (uint8) as PAYOFF_MAP_DATASET.
PAYOFF_OPTIONS = {
    "payoff_history_every": (0, _count),
    "payoff_max_distance": (None, lambda v: v),
    "payoff_map_final": (False, bool),
}


# The pair-map record's options (pairmap.py), class attributes of SPGG in a table of their own as the
# payoff record's are.  name -> (default, conversion).  pair_map_history_every = k > 0: record the 2-D pair
# maps of the fields of pair_map_fields -- a tuple of (a, b) pairs of "coop" and "flip" -- at every
# displacement up to pair_map_max_distance (None: min(L // 2, 32)) at t = 1, 1+k, ... on the device and
# write pair_map_history_iters, one pair_map_<a>_<b>_history per pair and pair_map_max_distance after the
# payoff datasets.
PAIR_MAP_OPTIONS = {
    "pair_map_history_every": (0, _count),
    "pair_map_max_distance": (None, lambda v: v),
    "pair_map_fields": ((("coop", "coop"),), lambda v: tuple(tuple(p) for p in v)),
}


def _tiled(v):
    return v if isinstance(v, bool) else (int(v) if v else False)


# The tiled cluster labelling's option, a class attribute of SPGG like the others in a table of its
# own.  name -> (default, BatchEngine.run keyword argument, conversion).  cluster_history_tiled: False:
# the in-run cluster record is written by the one-workgroup kernel (lattices up to side 200); True: by
# spgg_clusters_tiled (any side) with the library's tile; an int: with that tile side (8 .. 200).  Needs
# cluster_history_every > 0; the datasets are the same.
CLUSTER_TILED_OPTIONS = {
    "cluster_history_tiled": (False, "clusters_tiled", _tiled),
}


def cluster_tiled_run_kwargs(values):
    """BatchEngine.run's clusters_tiled keyword argument from option values (a mapping; absent: default)."""
    return {kw: conv(values.get(name, default)) for name, (default, kw, conv) in CLUSTER_TILED_OPTIONS.items()}


def dwell_option_values(values):
    """(dwell_every, dwell_fields) from option values (a mapping; absent: default)."""
    every, fields = (conv(values.get(name, default)) for name, (default, conv) in DWELL_OPTIONS.items())
    if fields and not every:
        raise ValueError("dwell_fields needs dwell_history_every > 0 (nothing is tracked otherwise)")
    return every, fields


def dwell_histories(eng, every, fields):
    """write_datasets' dwell_hist of every replica of a run(dwell_every=every): the engine's
    dwell_histories, with `fields` also the per-agent fields of the final state; None without."""
    if not every:
        return None
    hist = eng.dwell_histories()
    if fields:
        for k, h in enumerate(hist):
            f = eng.dwell_fields(k)
            h.update({name: f[key] for name, key in zip(DWELL_FIELD_DATASETS, ("flip_count", "strategy_age",
                                                                               "cooperation_frequency"))})
    return hist


def policy_option_values(values):
    """(BatchEngine.run's policy keyword arguments, policy_map_final) from option values (a mapping;
    absent: default)."""
    every, bins, gap_range, final = (conv(values.get(name, default)) for name, (default, conv) in POLICY_OPTIONS.items())
    if final and not every:
        raise ValueError("policy_map_final needs policy_history_every > 0 (nothing is recorded otherwise)")
    return dict(policy_every=every, policy_bins=bins, policy_gap_range=gap_range), final


def policy_histories(eng, run_kw, map_final):
    """write_datasets' policy_hist of every replica of a run(**run_kw): the engine's policy_histories,
    with map_final also the final state's map; None without the record."""
    if not run_kw["policy_every"]:
        return None
    hist = eng.policy_histories()
    if map_final:
        for k, h in enumerate(hist):
            h[POLICY_MAP_DATASET] = eng.policy_map(k)
    return hist


def payoff_option_values(values):
    """(BatchEngine.run's payoff keyword arguments, payoff_map_final) from option values (a mapping;
    absent: default)."""
    every, max_d, final = (conv(values.get(name, default)) for name, (default, conv) in PAYOFF_OPTIONS.items())
    if (final or max_d is not None) and not every:
        raise ValueError("payoff_max_distance and payoff_map_final need payoff_history_every > 0 (nothing is "
                         "recorded otherwise)")
    return dict(payoff_every=every, payoff_max_d=max_d), final


def payoff_histories(eng, run_kw, map_final):
    """write_datasets' payoff_hist of every replica of a run(**run_kw): the engine's payoff_histories,
    with map_final also the final state's map; None without the record."""
    if not run_kw["payoff_every"]:
        return None
    hist = eng.payoff_histories()
    if map_final:
        for k, h in enumerate(hist):
            h[PAYOFF_MAP_DATASET] = eng.payoff_map(k)
    return hist


def pair_map_option_values(values):
    """BatchEngine.run's pair-map keyword arguments from option values (a mapping; absent: default)."""
    every, max_d, fields = (conv(values.get(name, default)) for name, (default, conv) in PAIR_MAP_OPTIONS.items())
    if max_d is not None and not every:
        raise ValueError("pair_map_max_distance needs pair_map_history_every > 0 (nothing is recorded otherwise)")
    return dict(pair_map_every=every, pair_map_max_d=max_d, pair_map_fields=field_pairs(fields))


def pair_map_histories(eng, run_kw):
    """write_datasets' pair_map_hist of every replica of a run(**run_kw): the engine's pair_map_histories;
    None without the record."""
    return eng.pair_map_histories() if run_kw["pair_map_every"] else None


def record_run_kwargs(values):
    """BatchEngine.run's record keyword arguments from option values (a mapping; absent: default)."""
    return {kw: conv(values.get(name, default)) for name, (default, kw, conv) in RECORD_OPTIONS.items()}


class SPGG:
    """Spatial Public Goods Game with RL, reputation and neighbor influence."""

    save_png = True  # strategy PNGs at snapshot iterations (spgg.py:552-559)
    # (the RECORD_OPTIONS, DWELL_OPTIONS, CLUSTER_TILED_OPTIONS, POLICY_OPTIONS, PAYOFF_OPTIONS and PAIR_MAP_OPTIONS are class attributes too, set
    # at their defaults below the class)

    def __init__(self, r=2, c=1, cost=0.5, K=0.1, L=50, iterations=1000,
                 num_of_strategies=2, population_type=0, S_in_one=None,
                 alpha=0.1, gamma=0.9, epsilon=0.5, epsilon_decay=0.995,
                 epsilon_min=0.01, influence_factor=1.0, use_second_order=True,
                 lambda_epsilon=0.01, delta_R_C=1, delta_R_D=1, R_min=-10,
                 R_max=10, reward_weight_payoff=1.0, rep_gain_C=0.5,
                 state_representation='reputation', algorithm='qlearning', **params):
        np.random.seed()  # spgg.py:98: entropy reseed of the global MT19937

        all_params = dict(locals(), **params)
        del all_params['self'], all_params['params']
        self.params = all_params
        for key in self.params:
            setattr(self, key, self.params[key])
        self.reward_weight_rep = 1 - self.reward_weight_payoff

        if isinstance(algorithm, str):
            self.algorithm = A.create_algorithm(algorithm, alpha, gamma, epsilon,
                                                epsilon_decay, epsilon_min, **params)
        elif A.is_operator(algorithm):
            # the plug-in point (spgg.py:115-116): one of the operators the device step
            # implements, this package's or the reference's own; a custom operator raises
            # ValueError here instead of running the built-in math (algorithms.operator_kind)
            A.operator_kind(algorithm)
            self.algorithm = algorithm
        else:
            raise ValueError(f"algorithm must be str or RLAlgorithm, got {type(algorithm)}")

        self.q_table = np.random.uniform(low=-0.01, high=0.01, size=(L, L, 2, 2))
        if hasattr(self.algorithm, 'initialize_q_tables'):
            self.algorithm.initialize_q_tables(self.q_table.shape)
            self.q_table = self.algorithm.get_combined_q_table()
        self.R = np.zeros((L, L))
        self.cache = {}
        self._Sn = S_in_one
        self.create_population()

        self.track_positions = track_positions(L)
        self.q_history = {pos: {'q_c': [], 'q_d': []} for pos in self.track_positions}
        self.it_records = []
        self.epsilon_history = []
        self.rep_avg_history = []
        self.influence_counts = []
        self.best_neighbor_type_history = []
        self.normlize_max = 4 * r
        self.normlize_min = r - 5
        max_pow = int(np.floor(np.log10(self.iterations)))  # noqa: F841 (spgg.py:152)
        self.snapshot_iters = set(SNAPSHOT_ITERS)
        self.folder = None

    def create_population(self):
        """spgg.py:158-164."""
        L = self.L
        if self._Sn is None:
            self._Sn = np.random.randint(0, 2, size=(L, L))
        self._S = [(self._Sn == j).astype(int) for j in range(self.num_of_strategies)]
        return self._S

    def generate_cache_key(self, *args):
        return hash(args)

    # -- run -----------------------------------------------------------------
    def _replica_params(self):
        alg = self.algorithm
        return ReplicaParams(
            r=self.r, c=self.c, cost=self.cost, alpha=self.alpha, gamma=self.gamma,
            epsilon=alg.epsilon, epsilon_decay=alg.epsilon_decay, epsilon_min=alg.epsilon_min,
            influence_factor=self.influence_factor, lambda_epsilon=self.lambda_epsilon,
            delta_R_D=self.delta_R_D, R_min=self.R_min, R_max=self.R_max,
            reward_weight_payoff=self.reward_weight_payoff, rep_gain_C=self.rep_gain_C,
            alg_alpha=alg.alpha, alg_gamma=alg.gamma)

    def run(self, filename):
        """Run the simulation on the GPU and write the datasets (spgg.py:325-637).

        Returns (final_coop_rate, final_def_rate, mean_payoff) as numpy float64.
        """
        kind = A.canonical_name(self.algorithm)
        L = self.L
        S0 = np.asarray(self._Sn)
        n0 = int(np.sum(S0 == 0))
        absorbing0 = n0 == 0 or n0 == L * L
        state_rep = self.state_representation
        if state_rep not in ('reputation', 'action'):
            if not absorbing0:  # the reference raises at the first get_state (spgg.py:309)
                raise ValueError(f"Unknown state_representation: {state_rep}. "
                                 f"Must be 'reputation' or 'action'")
            state_rep = 'reputation'
        g = np.random.get_state()
        tables = None
        if kind == "double_qlearning":
            tables = (np.asarray(self.algorithm.q_table_1, dtype=np.float64),
                      np.asarray(self.algorithm.q_table_2, dtype=np.float64))
        init = InitState(Q=np.asarray(self.q_table, dtype=np.float64), S=S0, tables=tables,
                         mt_key=np.asarray(g[1], dtype=np.uint32), mt_pos=int(g[2]))
        iters = int(self.iterations)
        eng = BatchEngine(L, max(iters, 1), [self._replica_params()],
                          use_second_order=bool(self.use_second_order),
                          state_representation=state_rep, rng="mt19937", init=[init],
                          algorithm=kind)
        if iters < 1:
            eng.T = 0
        snapshots_dir = os.path.join(self.folder, 'plots', 'snapshots') if self.folder else 'snapshots'
        os.makedirs(snapshots_dir, exist_ok=True)
        try:
            records = record_run_kwargs({name: getattr(self, name) for name in RECORD_OPTIONS})
            dwell_every, dwell_fields = dwell_option_values({name: getattr(self, name) for name in DWELL_OPTIONS})
            tiled = cluster_tiled_run_kwargs({name: getattr(self, name) for name in CLUSTER_TILED_OPTIONS})
            policy_kw, policy_map = policy_option_values({name: getattr(self, name) for name in POLICY_OPTIONS})
            payoff_kw, payoff_map = payoff_option_values({name: getattr(self, name) for name in PAYOFF_OPTIONS})
            pair_map_kw = pair_map_option_values({name: getattr(self, name) for name in PAIR_MAP_OPTIONS})
            eng.run(snapshots=True, png=self.save_png, dwell_every=dwell_every, **records, **tiled, **policy_kw,
                    **payoff_kw, **pair_map_kw)
            hist = eng.histories()[0]
            clusters = eng.cluster_sizes(0)   # labelled on the device (over many workgroups above side 200)
            record_hists = {arg: h and h[0] for arg, h in record_histories(eng, records).items()}
            dwell_hist = dwell_histories(eng, dwell_every, dwell_fields)
            policy_hist = policy_histories(eng, policy_kw, policy_map)
            payoff_hist = payoff_histories(eng, payoff_kw, payoff_map)
            pair_map_hist = pair_map_histories(eng, pair_map_kw)
            Q, R, S = eng.final_state(0)
            tables = eng.final_tables(0) if kind == "double_qlearning" else None
            last = eng.last_iteration(0)
            P = eng.payoff_at(last)[0] if last >= 1 else None
            key, pos = eng.mt_state_host(0)
            m = len(hist["epsilon_history_final"])
            eps_after = float(eng.eps_host[0, m + 1]) if m > 0 else None
            snaps, frames = eng.snapshots[0], eng.png_frames[0]
        finally:
            eng.close()

        if self.save_png and frames:
            _write_pngs(frames, snapshots_dir)

        # state after the run, as the reference leaves it
        self.q_table, self.R, self._Sn = Q, R, S
        if tables is not None:  # the operator's own tables (spgg.py:496-502)
            self.algorithm.q_table_1, self.algorithm.q_table_2 = tables
        self._S = [(S == j).astype(int) for j in range(self.num_of_strategies)]
        self.cache = {}
        if P is not None:
            self.P = P
        if eps_after is not None:
            self.algorithm.epsilon = eps_after
            self.epsilon = eps_after
        np.random.set_state((g[0], key, pos, g[3], g[4]))

        # the datasets last: the reference fills its file after the loop, so a write
        # error (duplicate tracked positions at L <= 2) leaves the state above in place
        write_datasets(filename, hist, snaps, S, R, self.R_min, self.R_max, self.track_positions,
                       clusters=clusters, dwell_hist=dwell_hist and dwell_hist[0],
                       policy_hist=policy_hist and policy_hist[0], payoff_hist=payoff_hist and payoff_hist[0],
                       pair_map_hist=pair_map_hist and pair_map_hist[0], **record_hists)

        S_coop = (S == 0).astype(int)
        S_def = (S == 1).astype(int)
        return (np.sum(S_coop) / (L * L), np.sum(S_def) / (L * L), np.mean(P))


for _name, (_default, _kw, _conv) in RECORD_OPTIONS.items():
    setattr(SPGG, _name, _default)
for _name, (_default, _conv) in DWELL_OPTIONS.items():
    setattr(SPGG, _name, _default)
for _name, (_default, _kw, _conv) in CLUSTER_TILED_OPTIONS.items():
    setattr(SPGG, _name, _default)
for _name, (_default, _conv) in POLICY_OPTIONS.items():
    setattr(SPGG, _name, _default)
for _name, (_default, _conv) in PAYOFF_OPTIONS.items():
    setattr(SPGG, _name, _default)
for _name, (_default, _conv) in PAIR_MAP_OPTIONS.items():
    setattr(SPGG, _name, _default)


HISTORY_DATASETS = ("it_records_final", "epsilon_history_final", "rep_avg_history_final",
                    "coop_rate_history", "switch_C_to_D", "switch_D_to_C",
                    "neighbor_influence_percent", "payoff_component_history",
                    "rep_component_history", "best_neighbor_second_order_percent",
                    "reputation_reward_ratio", "avg_reward_C_history", "avg_reward_D_history")


CLUSTER_DATASETS = ("cluster_history_iters", "cluster_count_history", "largest_cluster_history",
                    "cd_bond_history")


CORRELATION_DATASETS = ("correlation_history_iters", "pair_count_rows_history", "pair_count_cols_history")


# the last four only with reputation_max_distance set (BatchEngine.reputation_histories)
REPUTATION_DATASETS = ("reputation_history_iters", "reputation_hist_history", "reputation_bin_edges",
                       "reputation_sum_history", "reputation_pair_rows_history", "reputation_pair_cols_history",
                       "reputation_unit")
OPTIONAL_DATASETS = REPUTATION_DATASETS[3:]
FLOAT_DATASETS = ("reputation_bin_edges", "reputation_unit")   # the other record datasets are int64


# per record kind: run()'s keyword that switches it on, the engine's getter, write_datasets' keyword, its datasets
RECORD_KINDS = (("clusters_every", "cluster_histories", "cluster_hist", CLUSTER_DATASETS),
                ("correlations_every", "correlation_histories", "correlation_hist", CORRELATION_DATASETS),
                ("reputation_every", "reputation_histories", "reputation_hist", REPUTATION_DATASETS))


def record_histories(eng, run_kwargs):
    """write_datasets' keyword -> the engine's per-replica histories of each record the run took
    (run_kwargs: record_run_kwargs' result), None for the others -- whose getter is not asked."""
    return {arg: getattr(eng, getter)() if run_kwargs[on] > 0 else None for on, getter, arg, _names in RECORD_KINDS}


def write_datasets(filename, hist, snaps, S, R, R_min, R_max, track_positions, clusters=None,
                   cluster_hist=None, correlation_hist=None, reputation_hist=None, dwell_hist=None, policy_hist=None,
                   payoff_hist=None, pair_map_hist=None):
    """The dataset layout `SPGG.run` writes (spgg.py:594-633): snapshots, the
    per-iteration histories, the never-filled tracked-position Q datasets and
    the final state.  Shared by SPGG.run and the batched sweep runner.

    clusters: the final cluster sizes (BatchEngine.cluster_sizes) instead of labelling S on the
    host here; cluster_hist: the in-run cluster record (BatchEngine.cluster_histories), written
    as the CLUSTER_DATASETS after the reference's own; correlation_hist: the in-run pair-count
    record (BatchEngine.correlation_histories), written as the CORRELATION_DATASETS after those;
    reputation_hist: the in-run reputation record (BatchEngine.reputation_histories), written as
    the REPUTATION_DATASETS it holds after those; dwell_hist: the in-run strategy dwell record
    (BatchEngine.dwell_histories), written as the DWELL_DATASETS after those, then the
    DWELL_FIELD_DATASETS it holds (int64; cooperation_frequency_final f64); policy_hist: the in-run
    policy record (BatchEngine.policy_histories), written as the POLICY_DATASETS after those (int64;
    policy_gap_bin_edges f64), then POLICY_MAP_DATASET (uint8) if it holds it; payoff_hist: the in-run
    payoff record (BatchEngine.payoff_histories), written as the PAYOFF_DATASETS after those (int64;
    payoff_values f64), then PAYOFF_PAIRS_DATASET (int64) and PAYOFF_MAP_DATASET (uint8) if it holds them;
    pair_map_hist: the in-run pair-map record (BatchEngine.pair_map_histories), written after those:
    pair_map_history_iters, one pair_map_<a>_<b>_history (rows, D + 1, 2 D + 1) per field pair and the scalar
    pair_map_max_distance, all int64.
    The defaults write the reference's file."""
    with open_writer(filename) as data_file:
        for i in sorted(snaps):
            Ri, Si = snaps[i]
            data_file.create_dataset(f"R_snapshot_{i}", data=Ri)
            h, bins = np.histogram(Ri, bins=20, range=(R_min, R_max))
            data_file.create_dataset(f"rep_hist_{i}", data=h)
            data_file.create_dataset(f"rep_bins_{i}", data=bins)
            data_file.create_dataset(f"Sn_snapshot_{i}", data=Si)
        for name in HISTORY_DATASETS:
            data_file.create_dataset(name, data=hist[name])
        for d in range(6):
            data_file.create_dataset(f"group_comp_d{d}_history", data=hist[f"group_comp_d{d}_history"])
        for grp in ("cooperators", "defectors"):
            for s in ("s0", "s1"):
                for a in ("c", "d"):
                    k = f"{grp}_q_{s}_{a}_history"
                    data_file.create_dataset(k, data=hist[k])
        for s in ("s0", "s1"):
            for a in ("c", "d"):
                k = f"avg_q_{s}_{a}_history"
                data_file.create_dataset(k, data=hist[k])
        for p_ in track_positions:  # never filled by the reference (spgg.py:345,620-622)
            data_file.create_dataset(f"q_c_pos_{p_[0]}_{p_[1]}_final", data=np.array([]))
            data_file.create_dataset(f"q_d_pos_{p_[0]}_{p_[1]}_final", data=np.array([]))
        data_file.create_dataset("Sn_final", data=S)
        data_file.create_dataset("R_final", data=R)
        h, bins = np.histogram(R, bins=20, range=(R_min, R_max))
        data_file.create_dataset("rep_hist_final", data=h)
        data_file.create_dataset("rep_bins_final", data=bins)
        data_file.create_dataset("cluster_sizes", data=cluster_sizes(S) if clusters is None
                                 else np.asarray(clusters, dtype=np.int64))
        for (_on, _getter, _arg, names), h in zip(RECORD_KINDS, (cluster_hist, correlation_hist, reputation_hist)):
            for name in names if h is not None else ():
                if name in h or name not in OPTIONAL_DATASETS:
                    data_file.create_dataset(name, data=np.asarray(
                        h[name], dtype=np.float64 if name in FLOAT_DATASETS else np.int64))
        for name in DWELL_DATASETS + DWELL_FIELD_DATASETS if dwell_hist is not None else ():
            if name in dwell_hist or name in DWELL_DATASETS:
                data_file.create_dataset(name, data=np.asarray(
                    dwell_hist[name], dtype=np.float64 if name == "cooperation_frequency_final" else np.int64))
        for name in POLICY_DATASETS if policy_hist is not None else ():
            data_file.create_dataset(name, data=np.asarray(
                policy_hist[name], dtype=np.float64 if name == "policy_gap_bin_edges" else np.int64))
        if policy_hist is not None and POLICY_MAP_DATASET in policy_hist:
            data_file.create_dataset(POLICY_MAP_DATASET, data=np.asarray(policy_hist[POLICY_MAP_DATASET], dtype=np.uint8))
        for name in PAYOFF_DATASETS if payoff_hist is not None else ():
            data_file.create_dataset(name, data=np.asarray(
                payoff_hist[name], dtype=np.float64 if name == "payoff_values" else np.int64))
        if payoff_hist is not None and PAYOFF_PAIRS_DATASET in payoff_hist:
            data_file.create_dataset(PAYOFF_PAIRS_DATASET, data=np.asarray(payoff_hist[PAYOFF_PAIRS_DATASET], dtype=np.int64))
        if payoff_hist is not None and PAYOFF_MAP_DATASET in payoff_hist:
            data_file.create_dataset(PAYOFF_MAP_DATASET, data=np.asarray(payoff_hist[PAYOFF_MAP_DATASET], dtype=np.uint8))
        if pair_map_hist is not None:
            maps = [name for name in pair_map_hist if name not in (PAIR_MAP_ITERS_DATASET, PAIR_MAP_DISTANCE_DATASET)]
            for name in [PAIR_MAP_ITERS_DATASET, *maps, PAIR_MAP_DISTANCE_DATASET]:
                data_file.create_dataset(name, data=np.asarray(pair_map_hist[name], dtype=np.int64))


def track_positions(L):
    """Positions whose Q the reference meant to track (spgg.py:143)."""
    return [(L // 2, L // 2), (L // 4, L // 4), (3 * L // 4, 3 * L // 4)]


def cluster_sizes(S):
    """Sizes of 4-connected non-periodic cooperator clusters, label order (spgg.py:631-633).

    One bincount instead of the reference's O(k*L^2) per-label comprehension.
    """
    from scipy.ndimage import label
    lab, n = label(S == 0)
    return np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)


def _write_pngs(frames, snapshots_dir):
    """Strategy snapshot images (spgg.py:14-20, 552-559)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib as mpl
        import matplotlib.pyplot as plt
    except Exception:  # noqa: BLE001 - matplotlib is optional for the hot path
        return
    cmap = mpl.colors.ListedColormap(["#eeeeee", "#111111"], N=2)
    for i, Sn in sorted(frames.items()):
        fig, ax = plt.subplots(figsize=(5, 5))
        ax.imshow(Sn, cmap=cmap, interpolation='nearest')
        ax.set_title(f"Strategy at iter={i}")
        ax.axis('off')
        fig.savefig(os.path.join(snapshots_dir, f"snapshot_{i}.png"))
        plt.close(fig)
