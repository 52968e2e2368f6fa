"""Every slot of the device history record against the exact record, under derived bounds.

stats[rep][t][SPGG_NSTAT] (BatchEngine.stats_folded) is compared, slot by slot and replica by
replica, with tests/_record.exact_record -- math.fsum over the oracle's per-agent terms -- under
tests/_record.bounds: counters, GMAX, the int8 path's SUMR and every slot the parameters or the
run's end force to zero bit-equal; f64 sums at the any-order bound (n - 1) u sum|x|; the slots
spgg_history_finalize regroups at an n-independent K u mag; the f32 NI percent at its own.  The
bounds are far below one agent's term (tests/test_record_bounds_cpu.py), so an agent lost from or
repeated in a sum -- an invalid-slot mask, a tile past the lattice edge, the prev-C / prev-D split,
a stripe, a slot finalised by the wrong launch -- fails here, where the derived means at 1e-5 pass.
S, R, Q and the stop iteration are held to the oracle too, to tell a record failure from a state one.

The cases are the smallest shapes that reach each record path."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from spgg_amd.engine import BatchEngine, ReplicaParams  # noqa: E402
from tests import _record as R  # noqa: E402
from tests._philox import EDGE_CASE, check_final  # noqa: E402

ALGS = ["qlearning", "sarsa", "expected_sarsa", "double_qlearning"]
START_SLOTS = (R.NCOOP, R.SUMP, R.SUMP_C, R.SUMP_D, R.SUMR)
STEP_SLOTS = tuple(k for k in range(R.NSTAT) if k not in START_SLOTS)


def _params(**kw):
    return ReplicaParams(**dict(R.BASE, **kw))


def _kw(p):
    return {k: getattr(p, k) for k in R.PARAM_KEYS}


def _record(rng, L, T, p, stream_id, M2, state, alg):
    """The exact record of replica p as the engine runs it: initial draws from RandomState(seed),
    then that stream (mt19937) or the Philox stream of (seed, stream id)."""
    if rng == "philox":
        return R.philox_record(L, T, _kw(p), p.seed, stream_id, M2, state, alg)
    return R.exact_record(_kw(p), L, T, M2, state, alg, rs=np.random.RandomState(p.seed))


def _force(monkeypatch, **env):
    for v in ("SPGG_APT", "SPGG_TILE", "SPGG_PERSIST", "SPGG_CACHE_MB", "SPGG_CHUNK", "SPGG_STREAMS",
              "SPGG_MT_CHUNK", "SPGG_MT_CHAINS", "SPGG_MT_PER_CHAIN", "SPGG_TILES_PER_STRIPE"):
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, v)


def _check_record(eng, st, k, rec, rows=None, skip=()):
    bad = R.mismatches(st[k], rec, R.bounds(rec, apt_max=4, rep_int8=eng.rep_int8), rows=rows, skip=skip)
    assert not bad, "replica %d: (t, slot, got, want, bound) %s%s" % (
        k, bad[:12], "" if len(bad) <= 12 else " ... %d in all" % len(bad))


def _check(eng, recs):
    """A finished (flushed) engine: every slot of every replica, then the final state."""
    assert eng.L in R.GPU_LATTICES      # (test_record_bounds_cpu.py holds the bounds at these lattices)
    st = eng.stats_folded().cpu().numpy()
    eng.all_stopped()
    assert st.shape == (len(recs), eng.T + 2, R.NSTAT)
    for k, rec in enumerate(recs):
        _check_record(eng, st, k, rec)
        assert int(eng.stopped[k]) == rec.stop_iter, (k, int(eng.stopped[k]), rec.stop_iter)
        check_final(eng.final_state(k), rec.final, k)
        if eng.double_q:
            q1, q2 = eng.final_tables(k)
            assert np.array_equal(q1, rec.final["tables"][0]) and np.array_equal(q2, rec.final["tables"][1]), k
    return st


def _run(L, T, reps, M2, state, alg, rng, recs, tile=None, **engine_kw):
    eng = BatchEngine(L, T, reps, use_second_order=M2, state_representation=state, rng=rng, algorithm=alg,
                      **engine_kw)
    try:
        if tile is not None:
            tile(eng)
        eng.run(snapshots=False)
        return _check(eng, recs)
    finally:
        eng.close()


# ---- a. run-time-width kernels: every operator, order, state, stream; one and four agents per thread
REPS_A = [(2.5, 0.0, 11), (3.0, 1.0, 12), (4.2, 0.5, 13), (1.0, 1.5, 14)]       # (r, kappa, seed)
ROWS_A = [(alg, True, "reputation") for alg in ALGS] + [("qlearning", False, "reputation"),
                                                         ("qlearning", True, "action")]


def _reps_a():
    return [_params(r=r, influence_factor=k, seed=s) for r, k, s in REPS_A]


@functools.lru_cache(maxsize=None)      # one oracle run per configuration, shared by both tilings; read only
def _want_a(rng, alg, M2, state):
    return [_record(rng, 18, 50, p, k, M2, state, alg) for k, p in enumerate(_reps_a())]


@pytest.mark.parametrize("apt", ["1", "max"])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
@pytest.mark.parametrize("alg,M2,state", ROWS_A)
def test_run_time_width_record(alg, M2, state, rng, apt, monkeypatch):
    _force(monkeypatch, SPGG_APT=apt)
    _run(18, 50, _reps_a(), M2, state, alg, rng, _want_a(rng, alg, M2, state))


# ---- b. odd lattice ----
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_odd_lattice_record(rng, monkeypatch):
    _force(monkeypatch)
    L, T = 13, 40
    reps = [_params(r=r, seed=s) for r, s in [(3.0, 31), (4.0, 32)]]
    _run(L, T, reps, True, "reputation", "qlearning", rng,
         [_record(rng, L, T, p, k, True, "reputation", "qlearning") for k, p in enumerate(reps)])


# ---- c. compile-time widths 20 and 40 ----
CTW_ROWS = [
    (False, "action", "qlearning", 1.0),
    (True, "reputation", "sarsa", 0.3),            # non-dyadic gain: f64 reputation planes
    (False, "reputation", "expected_sarsa", 0.3),
    (True, "action", "double_qlearning", 1.0),
    (False, "reputation", "double_qlearning", 0.3),
    (True, "reputation", "qlearning", 1.0),
]


def _ctw(L, apt, M2, state, alg, gain, monkeypatch, want_tile):
    _force(monkeypatch, SPGG_APT=apt)
    T = 40
    reps = [_params(seed=s, rep_gain_C=gain, r=3.0 + 0.4 * s) for s in (5, 6)]
    recs = [_record("philox", L, T, p, k, M2, state, alg) for k, p in enumerate(reps)]
    assert all(rec.rep_dyadic == (gain == 1.0) for rec in recs)
    _run(L, T, reps, M2, state, alg, "philox", recs, want_tile)


@pytest.mark.parametrize("M2,state,alg,gain", [r for r in CTW_ROWS if r[2] != "double_qlearning"])
def test_width_20_tiles_record(M2, state, alg, gain, monkeypatch):
    """L = 60, two agents per thread (Double-Q has no compile-time width 20)."""
    def tile(eng):
        assert eng.tile[0] == 20, eng.tile
        assert eng.rep_int8 == (gain == 1.0)

    _ctw(60, "2", M2, state, alg, gain, monkeypatch, tile)


@pytest.mark.parametrize("M2,state,alg,gain", CTW_ROWS)
def test_width_40_tiles_record(M2, state, alg, gain, monkeypatch):
    """L = 120, four agents per thread: 40 x 24 tiles, 64 of a workgroup's 1024 slots invalid."""
    def tile(eng):
        if alg != "double_qlearning":       # Double-Q tiles hold <= 512 agents: run-time width
            assert eng.tile == (40, 24), eng.tile
        assert eng.rep_int8 == (gain == 1.0)

    _ctw(120, "max", M2, state, alg, gain, monkeypatch, tile)


# ---- d. tiles that do not divide L: cells outside the lattice must not reach a sum ----
@pytest.mark.parametrize("M2", [False, True])
def test_tiles_not_dividing_the_lattice_record(M2, monkeypatch):
    """L = 80, four agents per thread: 27 x 27 tiles, the last tile row and column past the edge."""
    _force(monkeypatch, SPGG_APT="max")
    L, T = 80, 30
    reps = [_params(r=r, seed=s) for r, s in [(3.0, 41), (4.4, 42)]]

    def tile(eng):
        assert 512 < eng.tile[0] * eng.tile[1] <= 1024 and L % eng.tile[0] and L % eng.tile[1], eng.tile

    _run(L, T, reps, M2, "reputation", "qlearning", "philox",
         [_record("philox", L, T, p, k, M2, "reputation", "qlearning") for k, p in enumerate(reps)], tile)


# ---- e. history stripes ----
def test_stripes_record_l1000(monkeypatch):
    """L = 1000: 1000 workgroups fold into 16 stripes per slot (GMAX: their maximum)."""
    _force(monkeypatch)
    L, T = 1000, 3
    p = _params(seed=5)

    def tile(eng):
        assert eng.stripes == 16, eng.stripes

    st = _run(L, T, [p], False, "reputation", "qlearning", "mt19937",
              [_record("mt19937", L, T, p, 0, False, "reputation", "qlearning")], tile)
    assert (st[0, 1:T + 1, R.GMAX] > 0).all()


# ---- f. replica groups and cache-blocked waves ----
def _reps_f():
    return [_params(r=1.5 + 0.4 * s, influence_factor=0.5 * (s % 3), seed=40 + s) for s in range(9)]


@functools.lru_cache(maxsize=None)
def _want_f():
    return [_record("philox", 30, 60, p, k, True, "reputation", "qlearning") for k, p in enumerate(_reps_f())]


@pytest.mark.parametrize("streams", [1, 3])
def test_replica_groups_record(streams, monkeypatch):
    _force(monkeypatch)

    def groups(eng):
        assert eng.G == streams, eng.G

    _run(30, 60, _reps_f(), True, "reputation", "qlearning", "philox", _want_f(), groups, streams=streams)


def test_cache_blocked_waves_record(monkeypatch):
    """The settings of test_gpu_parity.test_cache_blocked_waves_match_concurrent_groups: a cache
    budget of 4 replicas' state (3 waves of the 9), turns of 7 iterations, 6 groups."""
    _force(monkeypatch)
    reps = _reps_f()
    probe = BatchEngine(30, 60, reps, use_second_order=True, rng="philox", streams=6)
    per_replica = probe.state_bytes_per_replica()
    probe.close()
    _force(monkeypatch, SPGG_CACHE_MB=repr(4 * per_replica / 2**20), SPGG_CHUNK="7")

    def waves(eng):
        assert eng.waves == 3 and eng.G == 6 and eng.resident == 2, (eng.waves, eng.G, eng.resident)

    _run(30, 60, reps, True, "reputation", "qlearning", "philox", _want_f(), waves, streams=6)


# ---- g. ragged step() calls: slot t - 1 is finalised by launch t, the last one by the flush ----
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_ragged_calls_record(rng, monkeypatch):
    _force(monkeypatch, SPGG_MT_CHUNK="16")
    L, T = 30, 40
    reps = [_params(r=r, seed=s) for r, s in [(3.0, 61), (4.4, 62)]]
    recs = [_record(rng, L, T, p, k, False, "reputation", "qlearning") for k, p in enumerate(reps)]
    assert all(rec.stop_iter == 0 for rec in recs)
    eng = BatchEngine(L, T, reps, use_second_order=False, rng=rng)
    try:
        if rng == "mt19937":
            assert eng.mt_layout[0] * eng.mt_layout[1] < T, eng.mt_layout      # the run crosses a generator chunk
        eng.step(1)
        eng.step(5)
        # launches 1 .. 6 are in: slots 0 .. 5 are complete; slot 6 lacks only what launch 7 adds
        # (phase 1a: the Q sums and the NI percent); slot 7 holds NCOOP; nothing later is touched
        mid = eng.stats_folded().cpu().numpy()
        for k, rec in enumerate(recs):
            _check_record(eng, mid, k, rec, rows=range(0, 6))
            _check_record(eng, mid, k, rec, rows=[6], skip=R.PENDING_SLOTS)
            assert not mid[k, 6, list(R.PENDING_SLOTS)].any(), k
            assert mid[k, 7, R.NCOOP] == rec.value[7, R.NCOOP] and not mid[k, 7, 1:].any(), k
            assert not mid[k, 8:].any(), k
        eng.step(T - 6)
        eng.flush()
        _check(eng, recs)
    finally:
        eng.close()


# ---- h. absorption and the eps edges ----
def _check_absorbing(st, k, rec, n):
    last = rec.last
    assert rec.stop_iter == last and st[k, last, R.NCOOP] in (0.0, float(n)), (k, last)
    assert not st[k, last, list(STEP_SLOTS)].any(), (k, "the absorbing iteration records its start only")
    assert not st[k, last + 1:].any(), (k, "slots past the last iteration")
    assert st[k, last, R.SUMP] != 0.0 and st[k, last - 1, R.SUMQ:R.SUMQ + 4].all(), k


def test_epsilon_edges_and_absorption_record(monkeypatch):
    _force(monkeypatch)
    L, T = EDGE_CASE["L"], EDGE_CASE["T"]
    reps = [ReplicaParams(**kw) for kw in EDGE_CASE["replicas"]]
    recs = [_record("philox", L, T, p, k, False, "reputation", "qlearning") for k, p in enumerate(reps)]
    stops = [rec.stop_iter for rec in recs]
    assert any(0 < s < T for s in stops), stops     # (test_philox_oracle_cpu.py keeps this true)
    st = _run(L, T, reps, False, "reputation", "qlearning", "philox", recs)
    for k, rec in enumerate(recs):
        if rec.stop_iter:
            _check_absorbing(st, k, rec, L * L)


def test_absorption_at_c_and_at_d_record(monkeypatch):
    """MT19937: one replica absorbs at all-C, one at all-D, one runs on."""
    _force(monkeypatch)
    L, T = 12, 80
    fast = dict(epsilon_decay=0.8, epsilon_min=0.0)
    reps = [_params(r=0.5, seed=51, **fast), _params(r=6.5, reward_weight_payoff=0.5, seed=52, **fast),
            _params(r=6.5, seed=53, **fast)]
    recs = [_record("mt19937", L, T, p, k, False, "reputation", "qlearning") for k, p in enumerate(reps)]
    ends = [(rec.stop_iter, rec.value[rec.last, R.NCOOP]) for rec in recs]
    assert 0 < ends[0][0] < T and ends[0][1] == 0 and 0 < ends[1][0] < T and ends[1][1] == L * L, ends
    assert ends[2][0] == 0, ends
    st = _run(L, T, reps, False, "reputation", "qlearning", "mt19937", recs)
    _check_absorbing(st, 0, recs[0], L * L)
    _check_absorbing(st, 1, recs[1], L * L)
    assert st[2, T + 1, R.NCOOP] == recs[2].value[T + 1, R.NCOOP] and not st[2, T + 1, 1:].any()


# ---- i. slots the parameters force to zero ----
def test_forced_zero_slots_record(monkeypatch):
    """w_P = 1 (w_rep = 0): SUM_WRR and SUM_RATIO_C are exactly 0; kappa = 0: SUM_PCT is exactly 0,
    while GMAX, NMD_POS and NMD_POS2 still hold the lattice's values (include/spgg_abi.h: they
    describe the rewards, whatever the influence factor does with them)."""
    _force(monkeypatch)
    L, T = 24, 30
    reps = [_params(reward_weight_payoff=1.0, seed=71), _params(influence_factor=0.0, seed=72),
            _params(reward_weight_payoff=1.0, influence_factor=0.0, seed=73)]
    recs = [_record("philox", L, T, p, k, True, "reputation", "qlearning") for k, p in enumerate(reps)]
    st = _run(L, T, reps, True, "reputation", "qlearning", "philox", recs)
    for k in (0, 2):
        assert not st[k][:, [R.SUM_WRR, R.SUM_RATIO_C]].any(), k
    for k in (1, 2):
        m = recs[k].last
        assert not st[k, :, R.SUM_PCT].any(), k
        assert (st[k, 1:m + 1, R.GMAX] > 0).all() and (st[k, 1:m + 1, R.NMD_POS] > 0).all(), k
        same = [R.GMAX, R.NMD_POS, R.NMD_POS2]
        assert np.array_equal(st[k][:, same], recs[k].value[:, same]), k
    assert st[0, 1:T + 1, R.SUM_PCT].all() and st[1, 1:T + 1, R.SUM_WRR].all()


# ---- j. persistent launches: the carried values cross a launch ----
@pytest.mark.parametrize("L,apt", [(60, "2"), (120, "max")])
@pytest.mark.parametrize("rng", ["philox", "mt19937"])
def test_persistent_launches_record(rng, L, apt, monkeypatch):
    """The two persistent instances at their smallest lattices -- two agents per thread at the
    compile-time tile width 20 (L >= 60), four at width 40 (L >= 120); below L = 60 the library has
    no compile-time-width tiling and so no persistent launch -- in step(7), step(T - 7): the values
    a workgroup carries in registers cross the launch boundary."""
    _force(monkeypatch, SPGG_PERSIST="1", SPGG_APT=apt)
    T = 40
    reps = [_params(r=r, seed=s) for r, s in [(3.0, 81), (4.4, 82)]]
    recs = [_record(rng, L, T, p, k, False, "reputation", "qlearning") for k, p in enumerate(reps)]
    eng = BatchEngine(L, T, reps, use_second_order=False, rng=rng)
    try:
        assert eng.persistent and eng.tile[0] == (20 if apt == "2" else 40), (eng.persist_capacity, eng.tile)
        eng.step(7)
        eng.step(T - 7)
        eng.flush()
        _check(eng, recs)
    finally:
        eng.close()
