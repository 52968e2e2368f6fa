"""The schedule of an in-run record (records.Record), the turn boundaries of BatchEngine.run
(records.next_boundary) and the drop-in's option table (spgg.RECORD_OPTIONS), without a GPU."""

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


def test_option_table():
    defaults = dict(cluster_history_every=0, cluster_history_periodic=False, correlation_history_every=0,
                    correlation_max_distance=None, reputation_history_every=0, reputation_history_bins=20,
                    reputation_max_distance=None)
    assert {n: d for n, (d, _kw, _conv) in spgg.RECORD_OPTIONS.items()} == defaults
    for name, value in defaults.items():
        assert getattr(spgg.SPGG, name) == value and type(getattr(spgg.SPGG, name)) is type(value), name
    assert spgg.record_run_kwargs({}) == dict(
        clusters_every=0, clusters_periodic=False, correlations_every=0, correlations_max_d=None,
        reputation_every=0, reputation_bins=20, reputation_max_d=None)
    got = spgg.record_run_kwargs(dict(cluster_history_every=None, cluster_history_periodic=1,
                                      correlation_history_every=2, correlation_max_distance=3,
                                      reputation_history_every="5", reputation_history_bins=9.0,
                                      reputation_max_distance=4))
    assert got == dict(clusters_every=0, clusters_periodic=True, correlations_every=2, correlations_max_d=3,
                       reputation_every=5, reputation_bins=9, reputation_max_d=4)
    assert type(got["clusters_periodic"]) is bool and type(got["reputation_bins"]) is int
    # each kind's switch and histories getter, in the order write_datasets writes them
    assert [k[:3] for k in spgg.RECORD_KINDS] == [
        ("clusters_every", "cluster_histories", "cluster_hist"),
        ("correlations_every", "correlation_histories", "correlation_hist"),
        ("reputation_every", "reputation_histories", "reputation_hist")]
    assert list(KINDS) == ["clusters", "correlations", "reputation"]
