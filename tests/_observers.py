"""The oracle's side of the seven in-run device records (clusters, correlations, reputation, dwell,
policy, payoff, pair_map): one oracle run per replica of a tests/_params.Batch gives S_t and R_t at the start of every
iteration, the policy rows (tests/_policy's, from the same run), the final state, the stop iteration
and (MT19937) the RandomState after the run; the expected datasets of a record are the existing host
models applied to those planes on the record's schedule.  The device has no part in any of it, and no
record is modelled here: tests/_clusters, _correlations, _reputation, _dwell, _policy, _payoff and _pairmap are.
NumPy only; no GPU, no engine is built (assert_all / assert_run read a finished one)."""
import dataclasses
import functools

import numpy as np

from oracle import philox as PH
from oracle import spgg_oracle as O
from spgg_amd import dwell as DW
from spgg_amd.pairmap import host_fields, host_pair_map
from spgg_amd.payoff import host_payoff_census, host_payoff_pairs
from spgg_amd.policy import host_policy_record, policy_bin_edges, split_row
from spgg_amd.records import host_pair_counts, reputation_bin_edges
from tests import _clusters as CL
from tests import _correlations as CO
from tests import _dwell as DM
from tests import _pairmap as PMT
from tests import _params as P
from tests import _payoff as PFT
from tests import _policy as PO
from tests import _reputation as RP
from tests._philox import check_final

KINDS = ("clusters", "correlations", "reputation", "dwell", "policy", "payoff", "pair_map")
GETTERS = dict(clusters="cluster_histories", correlations="correlation_histories", reputation="reputation_histories",
               dwell="dwell_histories", policy="policy_histories", payoff="payoff_histories", pair_map="pair_map_histories")
# the settings of tests/test_gpu_records_layouts.py: pairwise different periods, none of which divides or is divided by
# the turn lengths 7 (SPGG_CHUNK of the waves layout) and 8 (SPGG_ENQ_CHUNK of the no_interleave layout) -- which
# 2, 4 and 7 would; tests/test_records_layouts_cpu.py holds what the schedule has to satisfy
SETTINGS = dict(clusters=dict(every=3, periodic=False, tiled=False), correlations=dict(every=6, max_d=3),
                reputation=dict(every=5, bins=9, max_d=2), dwell=dict(every=9),
                policy=dict(every=11, bins=PO.BINS, gap_range=PO.GAP_RANGE), payoff=dict(every=13, max_d=2),
                pair_map=dict(every=10, max_d=2, fields=(("coop", "coop"), ("flip", "coop"))))


def settings(t0=1, scale=1, only=KINDS, **over):
    """SETTINGS for a run that starts at t0, the periods times `scale`, the kinds in `only`; a keyword
    per kind updates that kind's settings."""
    out = {k: dict(SETTINGS[k], **over.get(k, {})) for k in KINDS if k in only}
    for k in out:
        if k not in over or "every" not in over[k]:
            out[k]["every"] *= scale
    out["t0"] = int(t0)
    return out


def run_kwargs(s):
    """BatchEngine.run's keyword arguments of a settings dict."""
    kw = {}
    if "clusters" in s:
        c = s["clusters"]
        kw.update(clusters_every=c["every"], clusters_periodic=c["periodic"], clusters_tiled=c["tiled"])
    if "correlations" in s:
        kw.update(correlations_every=s["correlations"]["every"], correlations_max_d=s["correlations"]["max_d"])
    if "reputation" in s:
        r = s["reputation"]
        kw.update(reputation_every=r["every"], reputation_bins=r["bins"], reputation_max_d=r["max_d"])
    if "dwell" in s:
        kw.update(dwell_every=s["dwell"]["every"])
    if "policy" in s:
        p = s["policy"]
        kw.update(policy_every=p["every"], policy_bins=p["bins"], policy_gap_range=p["gap_range"])
    if "payoff" in s:
        kw.update(payoff_every=s["payoff"]["every"], payoff_max_d=s["payoff"]["max_d"])
    if "pair_map" in s:
        m = s["pair_map"]
        kw.update(pair_map_every=m["every"], pair_map_max_d=m["max_d"], pair_map_fields=m["fields"])
    return kw


@dataclasses.dataclass
class Trajectory:
    S: dict             # t -> S_t (L, L) uint8, 0 = C: t = 1 .. last, and last + 1 for a replica still running
    R: dict             # t -> R_t (L, L) float64
    policy: PO.Expected  # the policy rows, planes and bare rows of the same run
    last: int           # iterations with a start record (the absorbing one included)
    stop_iter: int
    final: dict         # the oracle's final state
    mt: tuple           # (key, pos) of the RandomState after the run (MT19937), else None
    unit: float         # the replica's dyadic reputation unit, or None
    row: dict
    L: int
    datasets: dict = None   # the oracle's own datasets of the run (no snapshots)

    @property
    def t_final(self):
        """The index of the state the run leaves: the absorbing iteration's, else the one after the last."""
        return self.last if self.stop_iter else self.last + 1


@functools.lru_cache(maxsize=None)      # one oracle run per replica, shared by every test that needs it; read only
def _trajectory(rng, L, T, M2, state, alg, seed, stream_id, frozen, bins, gap_range, policy_at):
    row = dict(frozen)
    p = P.oracle_params(row, L, T, M2, state, alg)
    edges = policy_bin_edges(gap_range, bins)
    rs = np.random.RandomState(seed)
    Q0, tables0 = O.init_tables(p, rs)          # as engine.reference_init draws them
    S0 = rs.randint(0, 2, size=(L, L))
    pol = PO.Expected({}, {}, {}, 0, 0, float(row["influence_factor"]), p, {})
    out = Trajectory({1: S0.astype(np.uint8)}, {1: np.zeros((L, L))}, pol, 0, 0, {}, None, P.unit_of(row), row, L)
    pol.rows[1], pol.planes[1] = host_policy_record(Q0, S0, O.get_state(S0, np.zeros((L, L)), p), bins, edges)
    ii, jj = np.indices((L, L))

    def on_step(i, S, R, Q, d):
        out.S[i + 1], out.R[i + 1] = np.array(S, dtype=np.uint8), np.array(R, dtype=np.float64)
        if policy_at is not None and i + 1 not in policy_at:
            return
        z = O.get_state(S, R, p)
        pol.rows[i + 1], pol.planes[i + 1] = host_policy_record(Q, S, z, bins, edges)
        bare = np.array(Q)
        bare[ii, jj, d["_old_states"], d["_actions"]] -= d["_nu"]
        pol.bare[i + 1] = host_policy_record(bare, S, z, bins, edges)[0]

    draws = None
    if rng == "philox":
        key = PH.philox_key(int(seed or 0), stream_id)
        draws = lambda i: PH.draws(key, L, i, alg)   # noqa: E731
    out.datasets, fin = O.run(p, rs, S_init=S0, Q_init=Q0, tables_init=tables0, collect_snapshots=False, on_step=on_step,
                              draws=draws)
    out.stop_iter = pol.stop_iter = int(fin["stop_iter"])
    out.last = pol.last = out.stop_iter if out.stop_iter else T
    out.final = pol.final = fin
    if out.t_final not in pol.rows:      # (a sparse policy_at: the state the run leaves is always held)
        pol.rows[out.t_final], pol.planes[out.t_final] = host_policy_record(
            fin["Q"], fin["S"], O.get_state(fin["S"], fin["R"], p), bins, edges)
    if rng == "mt19937":
        st = rs.get_state()
        out.mt = (np.asarray(st[1], dtype=np.uint32), int(st[2]))
    assert sorted(out.S) == list(range(1, out.t_final + 1)), (out.last, out.stop_iter)
    return out


def expected(b, bins=PO.BINS, gap_range=PO.GAP_RANGE, policy_at=None):
    """[Trajectory] of the replicas of a tests/_params.Batch, as the engine runs them: replica k seeded
    b.seeds[k] and (Philox) drawing stream k.  policy_at: the iterations whose policy rows are kept (a long
    run's: two host models per iteration are a third of its cost), None: all."""
    at = None if policy_at is None else frozenset(int(t) for t in policy_at)
    return [_trajectory(b.rng, b.L, b.T, b.M2, b.state, b.alg, s, k if b.rng == "philox" else 0, PO._freeze(row), bins,
                        gap_range, at) for k, (row, s) in enumerate(zip(b.rows, b.seeds))]


def iters(e, every, t0):
    return np.arange(t0, e.last + 1, every, dtype=np.int64)


def _stack(rows, shape, dtype=np.int64):
    return np.array(rows, dtype=dtype).reshape((len(rows),) + shape)


# ---- one row of every kind from a pair of planes: the existing host models, nothing else -------------------------------
def clusters_row(S, s):
    return np.array(CL.expected_record(S, s["periodic"]), dtype=np.int64)


def correlations_row(S, s):
    want = CO.expected_pair_counts((np.asarray(S) & 1) == 0, s["max_d"])
    assert np.array_equal(want, host_pair_counts(S, s["max_d"]))        # the package's host path says the same
    return want


def reputation_row(e, S, R, s):
    """(hist (2, bins), pair sums (2 D + 3,) in units of the replica's rep_unit, or None without max_d)."""
    hist = RP.expected_hist(S, R, s["bins"], e.row["R_min"], e.row["R_max"])
    if s["max_d"] is None:
        return hist, None
    K = R / e.unit
    assert np.array_equal(K, np.round(K)) and np.abs(K).max() <= 128      # the stored bytes, exactly
    total, rows, cols = RP.expected_pair_sums(K.astype(np.int64), s["max_d"])
    return hist, np.concatenate([[total], rows, cols])


def kind_row(e, kind, s, t):
    """The row of `kind` the models give on the planes of iteration t, flattened (not of dwell and policy, which
    are no function of the planes of one iteration)."""
    if kind == "clusters":
        return clusters_row(e.S[t], s)
    if kind == "correlations":
        return correlations_row(e.S[t], s).ravel()
    if kind == "reputation":
        h, r = reputation_row(e, e.S[t], e.R[t], s)
        return h.ravel() if r is None else np.concatenate([h.ravel(), r])
    if kind == "payoff":
        pairs = [] if s["max_d"] is None else [host_payoff_pairs(e.S[t], s["max_d"])]
        return np.concatenate([host_payoff_census(e.S[t])[0]] + pairs)
    if kind == "pair_map":
        f = host_fields(PMT.oracle_bytes(e, t), t)
        return np.concatenate([host_pair_map(f[a], f[b], s["max_d"]).ravel() for a, b in s["fields"]])
    raise ValueError(kind)


# ---- the datasets of the *_histories getters -----------------------------------------------------------------------------
def datasets(e, kind, s, t0=1):
    """What the kind's *_histories() getter gives for the replica under the settings s, from t0 on."""
    its = iters(e, s["every"], t0)
    m = len(its)
    if kind == "clusters":
        r = _stack([clusters_row(e.S[int(t)], s) for t in its], (3,))
        return dict(cluster_history_iters=its, cluster_count_history=r[:, 0], largest_cluster_history=r[:, 1],
                    cd_bond_history=r[:, 2])
    if kind == "correlations":
        D = s["max_d"]
        r = _stack([correlations_row(e.S[int(t)], s) for t in its], (2, D + 1))
        return dict(correlation_history_iters=its, pair_count_rows_history=r[:, 0], pair_count_cols_history=r[:, 1])
    if kind == "reputation":
        bins, D = s["bins"], s["max_d"]
        got = [reputation_row(e, e.S[int(t)], e.R[int(t)], s) for t in its]
        d = dict(reputation_history_iters=its, reputation_hist_history=_stack([h for h, _ in got], (2, bins)),
                 reputation_bin_edges=reputation_bin_edges(e.row["R_min"], e.row["R_max"], bins))
        assert np.array_equal(d["reputation_bin_edges"], RP.edges_of(e.row["R_min"], e.row["R_max"], bins))
        if D is not None:
            r = _stack([p for _, p in got], (2 * D + 3,))
            d.update(reputation_sum_history=r[:, 0], reputation_pair_rows_history=r[:, 1:D + 2],
                     reputation_pair_cols_history=r[:, D + 2:], reputation_unit=np.float64(e.unit))
        return d
    if kind == "dwell":
        r = _stack([DM.of_replica(e.S, e.last, t0, int(t))[0] for t in its], (DM.SLOTS,))
        return dict(dwell_history_iters=its, dwell_ref_iteration=np.int64(t0),
                    persistence_history=r[:, [DM.NEVER, DM.NEVER_C]], autocorrelation_history=r[:, [DM.SAME, DM.BOTH_C, DM.NCOOP]],
                    flip_total_history=r[:, DM.FLIPS], cooperator_time_history=r[:, DM.COOP_TIME],
                    strategy_age_hist_history=r[:, DM.AGE0:].reshape(m, 2, DM.AGE_BINS))
    if kind == "policy":
        its2, rows = (its, np.zeros((0, 21 + 4 * (s["bins"] + 2)), dtype=np.int64)) if m == 0 else \
            PO.history_rows(e.policy, s["every"], t0)
        assert np.array_equal(its, its2)
        counts, bonds, gaps = split_row(rows, s["bins"])
        return dict(policy_history_iters=its, policy_count_history=counts, policy_bond_history=bonds,
                    policy_gap_hist_history=gaps, policy_gap_bin_edges=policy_bin_edges(s["gap_range"], s["bins"]))
    if kind == "payoff":
        return PFT.datasets(e, s["every"], s["max_d"], t0)
    if kind == "pair_map":
        return PMT.datasets(e, s["every"], s["max_d"], s["fields"], t0)
    raise ValueError(kind)


def final_dwell(e, t0=1):
    """(row, fields (3, n), cooperation_frequency (n,)) of the state the run leaves."""
    tf = e.t_final
    row, f = DM.of_replica(e.S, tf, t0, tf)
    return row, f, f[2] / np.float64(max(tf, t0) - t0 + 1)


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def _compare(k, kind, got, want):
    assert list(got) == list(want), (k, kind, list(got), list(want))
    its = want[next(iter(want))]
    for name, w in want.items():
        g, w = np.asarray(got[name]), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (f"replica {k}", kind, name, g.dtype, g.shape, w.dtype, w.shape)
        if np.array_equal(g, w):
            continue
        if w.ndim and w.shape[0] == len(its) and not name.endswith("_edges"):
            bad = np.nonzero((g != w).reshape(len(its), -1).any(axis=1))[0]
            raise AssertionError((f"replica {k}", kind, name, "iterations", its[bad][:8].tolist(), "got",
                                  g[bad[0]].ravel().tolist(), "want", w[bad[0]].ravel().tolist()))
        raise AssertionError((f"replica {k}", kind, name, g.tolist(), w.tolist()))


def assert_all(eng, expected, s, kinds=None):
    """Every dataset of every armed record of a finished engine, its dtype and shape, and the final-state
    read-outs of dwell and policy, against the oracle's side; exact.  kinds: only these of the settings' kinds."""
    t0 = s.get("t0", 1)
    assert len(expected) == eng.R
    assert sorted(k for k in eng.records) == sorted(k for k in KINDS if k in s), (sorted(eng.records), sorted(s))
    if kinds is not None:
        s = {k: v for k, v in s.items() if k in kinds}
    for kind in KINDS:
        if kind not in s:
            continue
        assert eng.records[kind].t0 == t0 and eng.records[kind].every == s[kind]["every"], (kind, eng.records[kind].t0)
        hist = getattr(eng, GETTERS[kind])()
        assert len(hist) == eng.R
        for k, e in enumerate(expected):
            _compare(k, kind, hist[k], datasets(e, kind, s[kind], t0))
    if "dwell" in s:
        assert eng.dwell_t_ref == t0
        rows = eng.dwell_record()
        assert rows.dtype == np.int64 and rows.shape == (eng.R, DW.DWELL_SLOTS)
        for k, e in enumerate(expected):
            row, f, freq = final_dwell(e, t0)
            assert np.array_equal(rows[k], row), (f"replica {k}", "dwell_record", np.nonzero(rows[k] != row)[0].tolist())
            got = eng.dwell_fields(k)
            assert sorted(got) == ["cooperation_frequency", "flip_count", "strategy_age"]
            for name, w in (("flip_count", f[0]), ("strategy_age", f[1])):
                assert got[name].dtype == np.int64 and got[name].shape == (eng.L, eng.L), (k, name)
                assert np.array_equal(got[name].ravel(), w), (f"replica {k}", "dwell_fields", name)
            assert got["cooperation_frequency"].dtype == np.float64
            assert np.array_equal(got["cooperation_frequency"].ravel(), freq), (f"replica {k}", "cooperation_frequency")
    if "policy" in s:
        bins, rng = s["policy"]["bins"], s["policy"]["gap_range"]
        for k, e in enumerate(expected):
            rec = eng.policy_record(k, bins, rng)
            got = np.concatenate([rec["counts"].ravel(), rec["bonds"], rec["gap_hist"].ravel()])
            want = e.policy.rows[e.t_final]
            assert got.dtype == np.int64 and np.array_equal(got, want), (f"replica {k}", "policy_record", got.tolist(), want.tolist())
            assert np.array_equal(rec["gap_bin_edges"], policy_bin_edges(rng, bins))
            m = eng.policy_map(k)
            assert m.dtype == np.uint8 and np.array_equal(m, e.policy.planes[e.t_final]), (f"replica {k}", "policy_map")


def assert_run(eng, expected):
    """The run itself is the oracle's: S, R, Q (Double-Q: both tables) and the stop iteration bit for bit,
    under MT19937 the device key the oracle's RandomState after the run."""
    for k, e in enumerate(expected):
        check_final(eng.final_state(k), e.final, k)
        if eng.double_q:
            q1, q2 = eng.final_tables(k)
            assert np.array_equal(q1, e.final["tables"][0]) and np.array_equal(q2, e.final["tables"][1]), (k, "tables")
        assert int(eng.stopped[k]) == e.stop_iter and eng.last_iteration(k) == e.last, (k, int(eng.stopped[k]), e.stop_iter)
        if e.mt is not None:
            key, pos = eng.mt_state_host(k)
            assert pos == e.mt[1] and np.array_equal(key, e.mt[0]), (k, "MT19937 key")


# ---- the guards of tests/test_records_layouts_cpu.py ----------------------------------------------------------------------
def pending_term_visible(e, s, t0=1):
    """A recorded t >= 2 at which the policy row without iteration t - 1's neighbour-influence term (the table the
    device holds between two launches) has other class counts, or None: tests/_policy.guards' rule, on recorded rows."""
    for t in iters(e, s["every"], t0):
        t = int(t)
        if t >= 2 and not np.array_equal(e.policy.rows[t][:16], e.policy.bare[t][:16]):
            return t
    return None


def wrong_plane_visible(e, kind, s, t0=1):
    """A recorded t >= 2 at which the row of iteration t - 1 differs from that of t (the record of S_{t-1} /
    R_{t-1}, or of the table one iteration earlier, would not pass), or None."""
    for t in iters(e, s["every"], t0):
        t = int(t)
        if t < 2:
            continue
        if kind == "dwell":
            if t - 1 < t0:
                continue
            a, b = DM.of_replica(e.S, e.last, t0, t)[0], DM.of_replica(e.S, e.last, t0, t - 1)[0]
        elif kind == "policy":
            a, b = e.policy.rows[t], e.policy.rows[t - 1]
        else:
            a, b = kind_row(e, kind, s, t), kind_row(e, kind, s, t - 1)
        if not np.array_equal(a, b):
            return t
    return None


# ---- the layouts of tests/test_gpu_records_layouts.py and their batches ------------------------------------------------------
def _cut(b, n):
    return b._replace(rows=b.rows[:n], seeds=b.seeds[:n])


def _b6(rng, kind="dyadic", alg="qlearning"):
    return _cut(P.batch_b(kind, alg, True, "reputation", rng), 6)


_RUNNER = dict(P.R.BASE, alg_alpha=None, alg_gamma=None)       # tests/test_gpu_parity._runner_params
# four replicas at r = 1.0 (defection takes over: the whole of group 0 absorbs near t = 300), eight at r = 3.6, the
# first of which stops exploring at once and weighs reputation as much as payoff (absorbs at all-C within two dozen
# iterations, in a group whose other three run to the end); the third group runs to the end
RETIRED_ROWS = ([dict(_RUNNER, r=1.0)] * 4 + [dict(_RUNNER, r=3.6, epsilon_decay=0.8, epsilon_min=0.0, reward_weight_payoff=0.5)]
                + [dict(_RUNNER, r=3.6)] * 7)
RETIRED_SEEDS = tuple(range(60, 64)) + tuple(range(70, 78))
RETIRED_CHUNK = 64


def retired_batch(rng):
    return P.Batch("retired", rng, 12, 900, False, "reputation", "qlearning", RETIRED_ROWS, RETIRED_SEEDS)


@dataclasses.dataclass
class Layout:
    batch: object                   # rng -> tests/_params.Batch
    settings: dict
    streams: object = None          # BatchEngine's streams argument
    env: dict = dataclasses.field(default_factory=dict)    # the forced tuning variables ("budget": see the GPU test)
    chunk: int = 256                # run()'s chunk
    first: int = 0                  # plain step()s before the run
    absorbing: bool = False
    sparse_policy: bool = False     # keep the policy rows of the recorded iterations (and the ones before them) only

    def expected(self, rng):
        """[Trajectory] of the layout's batch under rng."""
        b = self.batch(rng)
        at = None
        if self.sparse_policy:
            due = range(self.settings["t0"], b.T + 1, self.settings["policy"]["every"])
            at = sorted({u for t in due for u in (t - 1, t) if u >= 1})
        return expected(b, policy_at=at)


LAYOUTS = {
    "one_group": Layout(_b6, settings()),
    "one_group_f64": Layout(lambda rng: _b6(rng, "mixed"), settings(reputation=dict(max_d=None))),
    "late_start": Layout(_b6, settings(t0=6), first=5),
    "groups": Layout(lambda rng: _b6(rng, alg="double_qlearning"), settings(), streams=3),
    "no_interleave": Layout(_b6, settings(), streams=3, env=dict(SPGG_INTERLEAVE="0", SPGG_ENQ_CHUNK="8")),
    "waves": Layout(lambda rng: _cut(P.batch_b("dyadic", "qlearning", True, "reputation", rng, L=30, T=61), 10), settings(),
                    streams=6, env=dict(SPGG_CACHE_MB="budget", SPGG_CHUNK="7")),
    "retired": Layout(retired_batch, settings(scale=8), streams=3, chunk=RETIRED_CHUNK, absorbing=True, sparse_policy=True),
    "persistent": Layout(lambda rng: P.batch_f(60)._replace(rng=rng),
                         settings(only=("clusters", "correlations", "reputation", "payoff", "pair_map"), clusters=dict(every=3),
                                  correlations=dict(every=4), reputation=dict(every=7)),
                         env=dict(SPGG_PERSIST="1", SPGG_APT="2"), chunk=5),
    "tiled_clusters": Layout(_b6, settings(clusters=dict(tiled=8, periodic=True))),
}
RNGS = ("mt19937", "philox")
CASES = [(name, rng) for name in LAYOUTS for rng in RNGS if (name, rng) != ("one_group_f64", "mt19937")]
