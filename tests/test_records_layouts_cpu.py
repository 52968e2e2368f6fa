"""The guards of tests/test_gpu_records_layouts.py, on the oracle alone (tests/_observers.py): its batches
are not absorbed away (and the retirement batch absorbs where it has to), a record taken from the planes
of iteration t - 1 instead of t is visible in every kind and replica, the periods interleave and avoid
the layouts' turn lengths, and the turns records.next_boundary cuts cover 1 .. T once and end at every
recorded iteration.  No GPU, no engine."""
import numpy as np
import pytest

from spgg_amd.records import Record, next_boundary
from tests import _observers as OB
from tests import _policy as PO

LAYOUT_NAMES = list(OB.LAYOUTS)
TURNS = dict(SPGG_CHUNK=7, SPGG_ENQ_CHUNK=8)      # the turn lengths the waves and no_interleave layouts force


def _case(name, rng):
    lay = OB.LAYOUTS[name]
    return lay, lay.batch(rng), lay.expected(rng)


def _records(s, T):
    return {k: Record(s[k]["every"], s["t0"], T) for k in OB.KINDS if k in s}


@pytest.mark.parametrize("name,rng", OB.CASES)
def test_batches_are_not_absorbed_away(name, rng):
    lay, b, exp = _case(name, rng)
    stops = [e.stop_iter for e in exp]
    assert all(e.last >= lay.settings["t0"] for e in exp), stops      # every replica is alive when the record starts
    if not lay.absorbing:
        assert 8 * sum(1 for s in stops if s) <= len(exp), stops      # the rule of tests/_policy.guards
        return
    T, chunk = b.T, lay.chunk
    bounds = np.linspace(0, len(exp), lay.streams + 1).round().astype(int)      # BatchEngine._create's groups
    groups = [stops[a:c] for a, c in zip(bounds[:-1], bounds[1:])]
    assert any(all(0 < s < T - 2 * chunk for s in g) for g in groups), groups            # a whole group, retired mid-run
    assert any(not any(g) for g in groups), groups                                      # a group that runs to T
    assert any(any(g) and not all(g) for g in groups), groups                           # an absorbed beside a live replica
    ends = {(int(np.all(e.final["S"] == 1)), e.stop_iter & 1) for e in exp if e.stop_iter}
    assert {a for a, _ in ends} == {0, 1}, ends                                         # absorbed at C and at D


@pytest.mark.parametrize("name,rng", OB.CASES)
def test_a_wrong_plane_is_visible(name, rng):
    lay, b, exp = _case(name, rng)
    s = lay.settings
    for kind in OB.KINDS:
        if kind not in s:
            continue
        for k, e in enumerate(exp):
            if len(OB.iters(e, s[kind]["every"], s["t0"])) >= 2:
                assert OB.wrong_plane_visible(e, kind, s[kind], s["t0"]) is not None, (k, kind)
    if "policy" in s:      # the table the device holds between two launches lacks the pending term
        seen = [OB.pending_term_visible(e, s["policy"], s["t0"]) for e in exp]
        assert any(seen) and not any(t for t, e in zip(seen, exp) if e.policy.kappa == 0.0), seen
        if lay.sparse_policy:      # a long run keeps the recorded rows only: every replica that has two shows it there
            assert all(t for t, e in zip(seen, exp) if len(OB.iters(e, s["policy"]["every"], s["t0"])) >= 2), seen
        else:                      # tests/_policy's guard, over every iteration
            PO.guards([e.policy for e in exp], lay.absorbing)


@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_the_schedule_interleaves(name):
    lay = OB.LAYOUTS[name]
    s, T = lay.settings, lay.batch("philox").T
    recs = _records(s, T)
    periods = [r.every for r in recs.values()]
    assert len(set(periods)) == len(periods) == (5 if name == "persistent" else 7), periods      # (dwell and policy: not there)
    assert set(recs) == set(OB.KINDS) - ({"dwell", "policy"} if name == "persistent" else set())
    due = {t: [k for k, r in recs.items() if t >= r.t0 and r.due(t)] for t in range(s["t0"], T + 1)}
    assert any(len(d) >= 3 for d in due.values())
    assert any(len(d) == 1 for d in due.values())
    assert any(not due[t] and not due[t + 1] for t in range(s["t0"], T)), due
    for var, turn in TURNS.items():
        if var in lay.env:
            assert int(lay.env[var]) == turn
            assert all(turn % p and p % turn for p in periods), (var, periods)
    if name == "one_group":      # the periods every layout but two runs avoid both turn lengths
        assert all(turn % p and p % turn for p in periods for turn in TURNS.values()), periods
    for k, r in recs.items():      # next_due is the first recorded iteration after t
        for t in range(s["t0"], T + 1):
            assert r.next_due(t) == min(u for u in range(t + 1, t + r.every + 1) if r.due(u)), (k, t)


@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_the_boundaries_are_right(name):
    """BatchEngine.run's loop, without an engine: the spans handed to step()."""
    lay = OB.LAYOUTS[name]
    s, T, chunk = lay.settings, lay.batch("philox").T, lay.chunk
    recs = list(_records(s, T).values())
    t = s["t0"]
    check_at, spans = t + chunk, []
    while t <= T:
        end = next_boundary(t, set(), check_at, T + 1, recs)
        assert t < end <= T + 1
        assert end == T + 1 or end == check_at or any(r.due(end) for r in recs), (t, end)
        spans.append((t, end))
        t = end
        if t < check_at and t <= T:
            continue
        check_at = t + chunk
    covered = [u for a, c in spans for u in range(a, c)]
    assert covered == list(range(s["t0"], T + 1))                      # 1 .. T, each once
    starts = {a for a, _ in spans}
    for r in recs:      # a row is written at the start of a turn: every recorded iteration starts one
        assert {int(u) for u in r.iters(T)} <= starts, (r.every, sorted(starts))
        assert r.rows == len(r.iters(T))
    ends = {c for _, c in spans}
    grid = set(range(s["t0"] + chunk, T + 1, chunk))                   # the stop-flag copies stay `chunk` iterations apart
    assert grid <= ends
    assert all(c in grid or c == T + 1 or any(r.due(c) for r in recs) for c in ends)
