"""The schedule of an in-run record (records.Record), the turn boundaries of BatchEngine.run
(records.next_boundary), the registry of the kinds with the drop-in's one option table
(records.KINDS, spgg.RECORD_OPTIONS) and the file layout write_datasets gives them, without a GPU."""

import numpy as np
import pytest

from spgg_amd import spgg
from spgg_amd.records import KINDS, Record, next_boundary


@pytest.mark.parametrize("t0", [1, 6])
@pytest.mark.parametrize("every", [1, 4, 7])
def test_schedule_against_a_walk(t0, every):
    for T in (t0 - 1, t0, 30, 40):
        rec = Record(every, t0, T)
        walk = [t for t in range(t0, T + 1) if (t - t0) % every == 0]   # t0, t0 + every, ... <= T
        assert rec.rows == max(1, len(walk)), (T, rec.rows)
        if T >= t0:
            assert rec.rows == (T - t0) // every + 1
        else:
            assert rec.rows == 1   # the run is already over: one row, never written
        for t in range(t0, T + 1):
            assert rec.due(t) == (t in walk), t
            later = [w for w in walk if w > t]
            assert rec.next_due(t) == (later[0] if later else walk[-1] + every), t
            assert t < rec.next_due(t) <= t + every
        assert [rec.row(t) for t in walk] == list(range(len(walk)))
        for last in {t0 - 1, min(t0, T), (t0 + T) // 2, T}:   # a replica's last iteration: never past T
            its = rec.iters(last)
            assert its.dtype == np.int64 and its.tolist() == [w for w in walk if w <= last], (T, last)
            assert np.array_equal(its, np.arange(t0, last + 1, every))


def _parent_nxt(t, stops, check_at, T, records):
    """The expression run() held before there was a record type, with (every, t0) per kind."""
    nxt = min([s for s in stops if s > t] + [check_at, T + 1])
    for every, t0 in records:
        if every:
            nxt = min(nxt, t + every - (t - t0) % every)
    return nxt


@pytest.mark.parametrize("stops", [set(), {1, 10, 11, 100, 101}])
@pytest.mark.parametrize("specs", [(), ((4, 1),), ((7, 1), (4, 6), (16, 3))])
def test_turn_boundaries_are_the_parents(stops, specs):
    T, chunk = 120, 32
    stops = {s for s in stops if s <= T + 1}
    t = start = max([t0 for _, t0 in specs], default=1)   # every record has started
    records = [Record(every, t0, T) for every, t0 in specs]
    check_at = t + chunk
    seen = []
    while t <= T:
        nxt = next_boundary(t, stops, check_at, T + 1, records)
        assert nxt == _parent_nxt(t, stops, check_at, T, specs), t
        assert t < nxt <= T + 1
        t = nxt
        seen.append(t)
        if not (t < check_at and t <= T and t not in stops):   # run(): a stop-flag copy here
            check_at = t + chunk
    assert seen[-1] == T + 1
    for rec in records:   # every recorded iteration of the run is a boundary
        assert {i for i in rec.iters(T).tolist() if i > start} <= set(seen)


def test_no_records_leave_the_stops_and_the_chunks():
    T, chunk = 100, 16
    for stops in (set(), {1, 10, 50, 51, 100}):
        t, check_at, seen = 1, 1 + chunk, []
        while t <= T:
            t = next_boundary(t, stops, check_at, T + 1)
            seen.append(t)
            check_at = t + chunk   # without records every boundary copies the stop flags
        want, t = [], 1
        while t <= T:   # the next stop, or chunk iterations on, or the end
            t = min([s for s in stops if s > t] + [t + chunk, T + 1])
            want.append(t)
        assert seen == want and seen[-1] == T + 1
        if not stops:
            assert seen == list(range(1 + chunk, T + 1, chunk)) + [T + 1]


# the one option table: (drop-in attribute, default, BatchEngine.run keyword or None, a raw value, its conversion)
OPTION_TABLE = [
    ("cluster_history_every", 0, "clusters_every", None, 0),
    ("cluster_history_periodic", False, "clusters_periodic", 1, True),
    ("cluster_history_tiled", False, "clusters_tiled", 8, 8),
    ("correlation_history_every", 0, "correlations_every", 2, 2),
    ("correlation_max_distance", None, "correlations_max_d", 3, 3),
    ("reputation_history_every", 0, "reputation_every", "5", 5),
    ("reputation_history_bins", 20, "reputation_bins", 9.0, 9),
    ("reputation_max_distance", None, "reputation_max_d", 4, 4),
    ("dwell_history_every", 0, "dwell_every", "4", 4),
    ("dwell_fields", False, None, 1, True),
    ("policy_history_every", 0, "policy_every", "3", 3),
    ("policy_history_bins", 32, "policy_bins", 16, 16),
    ("policy_history_gap_range", 2.0, "policy_gap_range", (-1, 2), (-1, 2)),
    ("policy_map_final", False, None, 1, True),
    ("payoff_history_every", 0, "payoff_every", "3", 3),
    ("payoff_max_distance", None, "payoff_max_d", 2, 2),
    ("payoff_map_final", False, None, 1, True),
    ("pair_map_history_every", 0, "pair_map_every", "3", 3),
    ("pair_map_max_distance", None, "pair_map_max_d", 2, 2),
    ("pair_map_fields", (("coop", "coop"),), "pair_map_fields", [["coop", "coop"], ["flip", "coop"]],
     (("coop", "coop"), ("flip", "coop"))),
]


def test_option_table():
    """All 20 options of the seven kinds live in spgg.RECORD_OPTIONS, in the registry's order."""
    from spgg_amd import sweep
    assert list(KINDS) == ["clusters", "correlations", "reputation", "dwell", "policy", "payoff", "pair_map"]
    assert all(issubclass(kind, Record) and kind.name == name for name, kind in KINDS.items())
    assert list(spgg.RECORD_OPTIONS) == [row[0] for row in OPTION_TABLE] and len(OPTION_TABLE) == 20
    assert list(spgg.RECORD_OPTIONS) == [o[0] for kind in KINDS.values() for o in kind.options]
    for name, default, run_kw, raw, want in OPTION_TABLE:
        d, kw, conv = spgg.RECORD_OPTIONS[name]
        assert d == default and type(d) is type(default) and kw == run_kw, name
        assert getattr(spgg.SPGG, name) == default and type(getattr(spgg.SPGG, name)) is type(default), name
        assert conv(raw) == want and type(conv(raw)) is type(want), name
        if name.endswith("_every"):
            assert conv(None) == 0
    assert [kind.options[0][1] for kind in KINDS.values()] == [
        "clusters_every", "correlations_every", "reputation_every", "dwell_every", "policy_every", "payoff_every",
        "pair_map_every"]      # each kind's switch first, in the order write_datasets writes the kinds
    assert [kind.getter for kind in KINDS.values()] == [
        "cluster_histories", "correlation_histories", "reputation_histories", "dwell_histories", "policy_histories",
        "payoff_histories", "pair_map_histories"]
    assert spgg.RECORD_OPTIONS["cluster_history_tiled"][2](True) is True and spgg.RECORD_OPTIONS["cluster_history_tiled"][2](0) is False

    defaults = {row[0]: row[1] for row in OPTION_TABLE}
    run_defaults = {row[2]: row[1] for row in OPTION_TABLE if row[2]}
    assert spgg.record_options({}) == (run_defaults, dict(dwell_fields=False, policy_map_final=False, payoff_map_final=False))
    assert len(run_defaults) == 17
    raw = {row[0]: row[3] for row in OPTION_TABLE}
    run_kw, extras = spgg.record_options(raw)
    assert run_kw == {row[2]: row[4] for row in OPTION_TABLE if row[2]}
    assert extras == dict(dwell_fields=True, policy_map_final=True, payoff_map_final=True)
    assert type(run_kw["clusters_periodic"]) is bool and type(run_kw["reputation_bins"]) is int

    kw = dict(raw, L=8, epsilon=0.2)      # the sweep takes all 20 out of the model overrides, converted
    assert sweep.pop_record_options(kw) == {row[0]: row[4] for row in OPTION_TABLE} and kw == dict(L=8, epsilon=0.2)
    assert sweep.pop_record_options({}) == defaults


def test_run_takes_the_kinds_keywords_and_no_other():
    """BatchEngine.run's head on a stand-in engine: another keyword is a TypeError, as a misspelt argument always
    was; then every kind's settings are checked, in registry order, with nothing allocated (the stand-in has no
    device: anything past the checks would fail otherwise)."""
    import types
    from spgg_amd.engine import BatchEngine
    eng = types.SimpleNamespace(L=16, persistent=True, rep_int8=False, clusters_max_side=200, correlations_max_side=200,
                                reputation_max_side=200, payoff_pairs_max_side=200, groups=[dict(r0=0, r1=1)], records={})
    with pytest.raises(TypeError, match="unexpected keyword argument 'cluster_every'"):
        BatchEngine.run(eng, cluster_every=3, reputation_bins=0, reputation_every=1)
    for kw, text in ((dict(clusters_every=-1, policy_every=-1), "clusters_every must be >= 0"),
                     (dict(reputation_every=2, reputation_max_d=3, dwell_every=2), "f64"),
                     (dict(dwell_every=2, policy_every=2), "dwell_every: this engine steps in persistent launches"),
                     (dict(dwell_every=-1), "dwell_every must be >= 0"),
                     (dict(policy_every=2, payoff_max_d=1), "policy_every: this engine steps in persistent launches"),
                     (dict(payoff_max_d=1), "payoff_max_d needs payoff_every > 0"),
                     (dict(pair_map_every=1, pair_map_max_d=9), "pair_map_max_d must lie in 0 .. L // 2 = 8")):
        with pytest.raises(ValueError, match=text):
            BatchEngine.run(eng, **kw)
        assert not eng.records


def test_record_histories_asks_only_the_armed_kinds():
    class Eng:
        def __getattr__(self, name):
            if name.endswith("_histories"):
                return lambda: [{name: k} for k in range(2)]
            if name in ("policy_map", "payoff_map"):
                return lambda k: (name, k)
            raise AssertionError(name)      # dwell_fields, or a getter of an unarmed kind

    run_kw, extras = spgg.record_options(dict(policy_history_every=2, policy_map_final=True, pair_map_history_every=3))
    got = spgg.record_histories(Eng(), run_kw, extras)
    assert list(got) == list(KINDS) and [n for n, h in got.items() if h is not None] == ["policy", "pair_map"]
    assert got["policy"] == [dict(policy_histories=k, policy_map_final=("policy_map", k)) for k in range(2)]
    assert got["pair_map"] == [dict(pair_map_histories=k) for k in range(2)]


# ---- the file layout: every kind, every optional dataset and the three final-state extras, for one replica ------------------
def _reference_hist():
    hist = {name: np.zeros(0) for name in spgg.HISTORY_DATASETS}
    hist.update({f"group_comp_d{d}_history": np.zeros(0) for d in range(6)})
    hist.update({f"{g}_q_{s}_{a}_history": np.zeros(0) for g in ("cooperators", "defectors", "avg")
                 for s in ("s0", "s1") for a in "cd"})
    return hist


def _every_kind(L=4, m=3, D=2, bins=5, pbins=3):
    """kind -> a history dict of synthetic int32 / float arrays of the right shapes: m rows, pair_map D = 1 with
    two field pairs."""
    def i(*shape):
        return np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape)
    its = np.arange(1, m + 1, dtype=np.int32)
    return dict(
        clusters=dict(cluster_history_iters=its, cluster_count_history=i(m), largest_cluster_history=i(m), cd_bond_history=i(m)),
        correlations=dict(correlation_history_iters=its, pair_count_rows_history=i(m, D + 1), pair_count_cols_history=i(m, D + 1)),
        reputation=dict(reputation_history_iters=its, reputation_hist_history=i(m, 2, bins),
                        reputation_bin_edges=np.linspace(-10, 10, bins + 1), reputation_sum_history=i(m),
                        reputation_pair_rows_history=i(m, D + 1), reputation_pair_cols_history=i(m, D + 1),
                        reputation_unit=np.float64(0.5)),
        dwell=dict(dwell_history_iters=its, dwell_ref_iteration=np.int64(1), persistence_history=i(m, 2),
                   autocorrelation_history=i(m, 3), flip_total_history=i(m), cooperator_time_history=i(m),
                   strategy_age_hist_history=i(m, 2, 27), flip_count_final=i(L, L), strategy_age_final=i(L, L),
                   cooperation_frequency_final=i(L, L) / 16.0),
        policy=dict(policy_history_iters=its, policy_count_history=i(m, 4, 2, 2), policy_bond_history=i(m, 5),
                    policy_gap_hist_history=i(m, 2, 2, pbins + 2), policy_gap_bin_edges=np.linspace(-2, 2, pbins + 1),
                    policy_map_final=i(L, L)),
        payoff=dict(payoff_history_iters=its, payoff_census_history=i(m, 2, 5, 26), payoff_bond_history=i(m, 103),
                    payoff_values=i(2, 26) / 7.0, payoff_pair_sums_history=i(m, 14), payoff_map_final=i(L, L)),
        pair_map={"pair_map_history_iters": its, "pair_map_max_distance": np.int64(1),
                  "pair_map_coop_coop_history": i(m, 2, 3), "pair_map_flip_coop_history": i(m, 2, 3)})


# (name, dtype, shape) of every record dataset in file order, after the reference's own
RECORD_FILE_LAYOUT = [
    ("cluster_history_iters", "int64", (3,)), ("cluster_count_history", "int64", (3,)),
    ("largest_cluster_history", "int64", (3,)), ("cd_bond_history", "int64", (3,)),
    ("correlation_history_iters", "int64", (3,)), ("pair_count_rows_history", "int64", (3, 3)),
    ("pair_count_cols_history", "int64", (3, 3)),
    ("reputation_history_iters", "int64", (3,)), ("reputation_hist_history", "int64", (3, 2, 5)),
    ("reputation_bin_edges", "float64", (6,)), ("reputation_sum_history", "int64", (3,)),
    ("reputation_pair_rows_history", "int64", (3, 3)), ("reputation_pair_cols_history", "int64", (3, 3)),
    ("reputation_unit", "float64", ()),
    ("dwell_history_iters", "int64", (3,)), ("dwell_ref_iteration", "int64", ()), ("persistence_history", "int64", (3, 2)),
    ("autocorrelation_history", "int64", (3, 3)), ("flip_total_history", "int64", (3,)),
    ("cooperator_time_history", "int64", (3,)), ("strategy_age_hist_history", "int64", (3, 2, 27)),
    ("flip_count_final", "int64", (4, 4)), ("strategy_age_final", "int64", (4, 4)),
    ("cooperation_frequency_final", "float64", (4, 4)),
    ("policy_history_iters", "int64", (3,)), ("policy_count_history", "int64", (3, 4, 2, 2)),
    ("policy_bond_history", "int64", (3, 5)), ("policy_gap_hist_history", "int64", (3, 2, 2, 5)),
    ("policy_gap_bin_edges", "float64", (4,)), ("policy_map_final", "uint8", (4, 4)),
    ("payoff_history_iters", "int64", (3,)), ("payoff_census_history", "int64", (3, 2, 5, 26)),
    ("payoff_bond_history", "int64", (3, 103)), ("payoff_values", "float64", (2, 26)),
    ("payoff_pair_sums_history", "int64", (3, 14)), ("payoff_map_final", "uint8", (4, 4)),
    ("pair_map_history_iters", "int64", (3,)), ("pair_map_coop_coop_history", "int64", (3, 2, 3)),
    ("pair_map_flip_coop_history", "int64", (3, 2, 3)), ("pair_map_max_distance", "int64", ()),
]
REFERENCE_TAIL = ["Sn_final", "R_final", "rep_hist_final", "rep_bins_final", "cluster_sizes"]


def test_file_layout_of_every_kind(tmp_path, monkeypatch):
    from spgg_amd import h5io
    monkeypatch.setenv("SPGG_H5_SINK", "npz")      # (the sink that keeps the order of writing)
    S, Rn = np.zeros((4, 4), dtype=np.int64), np.zeros((4, 4))
    kinds = _every_kind()
    fn = str(tmp_path / "all.h5")
    spgg.write_datasets(fn, _reference_hist(), {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64),
                        records=kinds)
    got = h5io.read_datasets(fn)
    names = list(got)
    own = names.index("cluster_sizes") + 1
    assert names[own - 5:own] == REFERENCE_TAIL
    assert [(n, str(got[n].dtype), got[n].shape) for n in names[own:]] == RECORD_FILE_LAYOUT
    for h in kinds.values():
        for name, want in h.items():
            assert np.array_equal(got[name], want), name
    spgg.write_datasets(fn, _reference_hist(), {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64))
    assert list(h5io.read_datasets(fn)) == names[:own]      # the reference's file
