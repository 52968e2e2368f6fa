"""The learned policy record (spgg_policy; BatchEngine.run(policy_every=), policy_record, policy_map)
against the oracle, bit for bit.

The expected row of iteration t is the host model (spgg_amd.policy.host_policy_record) applied to the
oracle's table, strategies and get_state at the start of t (tests/_policy.py).  Between two step
launches the device's Q buffer lacks iteration t-1's neighbour-influence term, which the kernel
rebuilds; tests/_policy.guards asserts, on the oracle's side, that every kappa != 0 replica has a
recorded row at which leaving the term out gives other class counts -- a kernel that read the buffer
as it stands fails there -- that all four classes and both states occur, and that the batches are
not absorbed away.  Integers, exact; the shapes are the smallest at which each part can go wrong."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from oracle import spgg_oracle as O  # noqa: E402
from spgg_amd import _lib, policy as PL, sweep as SW  # noqa: E402
from spgg_amd.engine import BatchEngine, ReplicaParams, reference_init, to_state_planes  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402
from tests import _params as P  # noqa: E402
from tests import _policy as PO  # noqa: E402
from tests import _record as R  # noqa: E402
from tests.test_gpu_record import _force  # noqa: E402

BINS, RANGE = PO.BINS, PO.GAP_RANGE


def _engine(b, **kw):
    reps = [P.replica_params(row, s) for row, s in zip(b.rows, b.seeds)]
    return BatchEngine(b.L, b.T, reps, use_second_order=b.M2, state_representation=b.state, rng=b.rng, algorithm=b.alg, **kw)


def _short(b, T=12, reps=None):
    n = len(b.rows) if reps is None else reps
    return b._replace(T=T, rows=b.rows[:n], seeds=b.seeds[:n])


def _state_row(eng, k, e, bins=BINS, gap_range=RANGE):
    """The host model on what final_state(k) returns."""
    Q, Rn, S = eng.final_state(k)
    return PL.host_policy_record(Q, S, O.get_state(S, Rn, e.params), bins, PL.policy_bin_edges(gap_range, bins))


def _check_history(eng, exp, every=1, bins=BINS):
    hist = eng.policy_histories()
    for k, e in enumerate(exp):
        its, rows = PO.history_rows(e, every)
        counts, bonds, gaps = PL.split_row(rows, bins)
        h = hist[k]
        assert np.array_equal(h["policy_history_iters"], its), (k, h["policy_history_iters"], its)
        for name, want in (("policy_count_history", counts), ("policy_bond_history", bonds), ("policy_gap_hist_history", gaps)):
            got = h[name]
            assert got.shape == want.shape and got.dtype == np.int64, (k, name, got.shape, want.shape)
            bad = np.nonzero((got != want).reshape(len(its), -1).any(axis=1))[0]
            assert bad.size == 0, (k, name, "iterations", its[bad].tolist(), got[bad[0]].ravel().tolist(),
                                   want[bad[0]].ravel().tolist())
        assert np.array_equal(h["policy_gap_bin_edges"], PL.policy_bin_edges(RANGE, bins))


def _check_state(eng, exp, t):
    """policy_record / policy_map of the state the engine is in (its next iteration: t) against the
    oracle's row of t (absorbed replicas: of their absorbing iteration)."""
    for k, e in enumerate(exp):
        tt = e.stop_iter if e.stop_iter and e.stop_iter < t else t
        rec = eng.policy_record(k, BINS, RANGE)
        got = np.concatenate([rec["counts"].ravel(), rec["bonds"], rec["gap_hist"].ravel()])
        assert np.array_equal(got, e.rows[tt]), (k, t, tt, got.tolist(), e.rows[tt].tolist())
        assert np.array_equal(eng.policy_map(k), e.planes[tt]), (k, t, tt)


def _run(b, every=1, look=None, absorbing=False, guard=True, **kw):
    exp = PO.expected(b)
    if guard:
        PO.guards(exp, absorbing)
    eng = _engine(b, **kw)
    try:
        if look:
            look(eng)
        eng.run(snapshots=False, policy_every=every, policy_bins=BINS, policy_gap_range=RANGE)
        _check_history(eng, exp, every)
        # after run(): the flushed table -- final_state's Q through the host model, and the oracle's
        _check_state(eng, exp, b.T + 1)
        for k, e in enumerate(exp):
            row, plane = _state_row(eng, k, e)
            rec = eng.policy_record(k, BINS, RANGE)
            assert np.array_equal(np.concatenate([rec["counts"].ravel(), rec["bonds"], rec["gap_hist"].ravel()]), row), k
            assert np.array_equal(eng.policy_map(k), plane), k
    finally:
        eng.close()
    return exp


# ---- operators, configurations, streams, reputation planes ------------------------------------------------
@pytest.mark.parametrize("M2,state", P.CONFIGS_B)
@pytest.mark.parametrize("alg", P.ALGS)
def test_every_operator_and_configuration_philox(alg, M2, state, monkeypatch):
    """B_ROWS["dyadic"]: the int8 reputation lattice, every parameter different in every replica."""
    _force(monkeypatch)
    _run(_short(P.batch_b("dyadic", alg, M2, state, "philox")), look=lambda eng: eng.rep_int8 or pytest.fail("f64 planes"))


@pytest.mark.parametrize("M2,state", P.CONFIGS_B)
@pytest.mark.parametrize("alg", ["qlearning", "double_qlearning"])
def test_f64_reputation_planes(alg, M2, state, monkeypatch):
    """B_ROWS["mixed"]: one free row puts the batch on the f64 reputation planes."""
    _force(monkeypatch)
    _run(_short(P.batch_b("mixed", alg, M2, state, "philox")), look=lambda eng: eng.rep_int8 and pytest.fail("int8 lattice"))


@pytest.mark.parametrize("alg", P.ALGS)
def test_every_operator_mt19937(alg, monkeypatch):
    _force(monkeypatch)
    _run(_short(P.batch_b("dyadic", alg, True, "reputation", "mt19937")))


EDGE_NAMES = ("kappa_1e-9", "kappa_25", "lambda_1e-12", "lambda_50")


def test_edge_rows(monkeypatch):
    """kappa = 1e-9 and 25, lambda_epsilon = 1e-12 and 50 (and the other EDGE rows beside them).  The
    guard holds for three of the four: the term of kappa = 1e-9 (at most 1e-9) is far below every gap
    of a dozen iterations, so that row alone could pass without it; it is there for its arithmetic."""
    _force(monkeypatch)
    b = _short(P.batch_c("int8", "qlearning", "philox"))
    names = list(P.EDGE_INT8)
    exp = PO.expected(b)
    for name in EDGE_NAMES:
        e = exp[names.index(name)]
        moved16 = any(not np.array_equal(e.rows[t][:16], e.bare[t][:16]) for t in range(2, e.last + 1))
        assert moved16 or name == "kappa_1e-9", name
    _run(b, guard=False)


# ---- shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M2", [False, True])
@pytest.mark.parametrize("L", [5, 13])
def test_small_and_odd_lattices(L, M2, monkeypatch):
    """L = 5: narrower than the window, every wrap aliases; L = 13: odd, replica planes unaligned."""
    _force(monkeypatch)
    _run(_short(P.batch_b("dyadic", "qlearning", M2, "reputation", "philox", L=L), reps=4))


@pytest.mark.parametrize("apt", ["1", "max"])
def test_agents_per_thread(apt, monkeypatch):
    """L = 18 stepped at one and at four agents per thread: the stored and the recomputed pending record."""
    _force(monkeypatch, SPGG_APT=apt)
    _run(_short(P.batch_b("dyadic", "double_qlearning", True, "reputation", "philox")))


@pytest.mark.parametrize("M2", [False, True])
def test_lattice_that_no_tile_divides(M2, monkeypatch):
    """L = 70: three observer tiles across (32, 32, 6) and nine down (8 x 8, 6)."""
    assert 70 % PL_TILE[0] and 70 % PL_TILE[1] and 70 // PL_TILE[0] >= 2 and 70 // PL_TILE[1] >= 2
    _force(monkeypatch)
    _run(_short(P.batch_b("mixed", "qlearning", M2, "reputation", "philox", L=70), reps=4))


PL_TILE = (32, 8)      # spgg_policy.h: kTileW x kTileH


@pytest.mark.parametrize("L,apt", [(60, "2"), (120, "max")])
@pytest.mark.parametrize("M2,state,alg,kind", P.CTW_ROWS[:2])
def test_compile_time_width_step_instances(L, apt, M2, state, alg, kind, monkeypatch):
    """L = 60 and 120: the step kernels of compile-time width and their recomputed record, T = 8."""
    _force(monkeypatch, SPGG_APT=apt)
    _run(_short(P.batch_d(L, M2, state, alg, kind), T=8, reps=3),
         look=lambda eng: eng.tile[0] == (20 if L == 60 else 40) or pytest.fail(str(eng.tile)))


def test_gmax_is_a_maximum_over_stripes(monkeypatch):
    """L = 1000: the history record has 16 stripes (tests/test_gpu_record.py), so the term's
    denominator is the maximum over them."""
    _force(monkeypatch)
    b = P.Batch("stripes", "mt19937", 1000, 3, False, "reputation", "qlearning", [dict(R.BASE, alg_alpha=None, alg_gamma=None)], (5,))
    _run(b, look=lambda eng: eng.stripes == 16 or pytest.fail(str(eng.stripes)), guard=False)
    e = PO.expected(b)[0]
    assert any(not np.array_equal(e.rows[t][:16], e.bare[t][:16]) for t in (2, 3))


@pytest.mark.parametrize("streams", [1, 3])
def test_replica_groups(streams, monkeypatch):
    _force(monkeypatch)
    _run(_short(P.batch_f(18)), look=lambda eng: eng.G == streams or pytest.fail(str(eng.G)), streams=streams)


def test_every_third_iteration(monkeypatch):
    _force(monkeypatch)
    _run(_short(P.batch_b("dyadic", "expected_sarsa", True, "reputation", "philox")), every=3)


# ---- states of the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,M2,state", [("qlearning", True, "reputation"), ("double_qlearning", True, "action"),
                                          ("sarsa", False, "reputation")])
def test_before_a_run_and_between_steps(alg, M2, state, monkeypatch):
    """t = 1 before any step: the initial table, the state without bit 4.  After step(k) without a
    flush: the pending path.  After flush(): the finalized table, the same row."""
    _force(monkeypatch)
    b = _short(P.batch_b("dyadic", alg, M2, state, "philox"))
    exp = PO.expected(b)
    PO.guards(exp)
    eng = _engine(b)
    try:
        _check_state(eng, exp, 1)
        for k in (3, 2, 1):
            eng.step(k)
            _check_state(eng, exp, eng.t)
        t = eng.t
        eng.flush()
        eng._final_cache = {}
        _check_state(eng, exp, t)
    finally:
        eng.close()


def test_narrow_gap_range_fills_both_outer_slots(monkeypatch):
    _force(monkeypatch)
    b = _short(P.batch_b("dyadic", "qlearning", True, "reputation", "philox"), reps=4)
    bins, rng = 5, (0.0, 0.3)
    exp = PO.expected(b, bins, rng)
    hs = [PL.split_row(e.rows[7], bins)[2] for e in exp]
    full = [k for k, h in enumerate(hs) if h[..., 0].sum() > 0 and h[..., -1].sum() > 0 and h[..., 1:-1].sum() > 0]
    assert len(full) >= 3, full       # both outer slots and the bins between them hold agents
    assert all(sum(h[sg, s, j] for h in hs) > 0 for sg in (0, 1) for s in (0, 1) for j in (0, bins + 1))
    eng = _engine(b)
    try:
        eng.step(6)
        for k, e in enumerate(exp):
            rec = eng.policy_record(k, bins, rng)
            got = np.concatenate([rec["counts"].ravel(), rec["bonds"], rec["gap_hist"].ravel()])
            assert np.array_equal(got, e.rows[7]), (k, got.tolist(), e.rows[7].tolist())
            assert rec["gap_hist"].sum(axis=(1, 2)).tolist() == [2 * rec["counts"][:, s].sum() for s in (0, 1)]
    finally:
        eng.close()


# ---- absorbed replicas: the plane and the table of the absorbing iteration ------------------------------------------
STOPS = (0, 3, 4, 6, 9)     # live; absorbed at an odd, an even iteration; at the first observed one; after both
TIMES = (6, 7)


@pytest.mark.parametrize("alg,M2", [("qlearning", False), ("double_qlearning", True)])
def test_absorbed_replicas_read_their_own_plane_and_table(alg, M2, monkeypatch):
    """The rule of tests/test_gpu_observed_plane.py: every replica holds two different lattices,
    stop_iter marks it live or absorbed at s, and the record of t is that of plane (tt - 1) & 1 with
    tt = s for s < t.  An absorbed replica's table is final in place: its kappa != 0 must not bring
    the pending term in.  The live replica has kappa = 0, so its table in place is T whatever its bits."""
    _force(monkeypatch)
    L, T, Rn = 5, 10, len(STOPS)
    rs = np.random.RandomState(31)
    S = ((rs.rand(2, Rn, L, L) < 0.45).astype(np.uint8) | (rs.randint(0, 16, (2, Rn, L, L)) << 1)).astype(np.uint8)
    tabs = rs.uniform(-1, 1, (2, Rn, L, L, 2, 2))
    dq = alg == "double_qlearning"
    Qb = np.stack([to_state_planes(tabs[0, k], tabs[1, k]) if dq else to_state_planes(tabs[0, k]) for k in range(Rn)])
    Tab = (tabs[0] + tabs[1]) * 0.5 if dq else tabs[0]
    reps = [ReplicaParams(**dict(R.BASE, influence_factor=0.0 if s == 0 else 1.0, seed=k)) for k, s in enumerate(STOPS)]
    init = [reference_init(L, np.random.RandomState(k), algorithm=alg) for k in range(Rn)]
    eng = BatchEngine(L, T, reps, use_second_order=M2, rng="philox", init=init, algorithm=alg)
    edges = PL.policy_bin_edges(RANGE, BINS)
    try:
        done = 0
        for t in TIMES:
            eng.step(t - 1 - done)
            done = t - 1
            torch.cuda.synchronize()
            eng.S.copy_(torch.from_numpy(S.reshape(2, Rn, L * L)).to(eng.dev))
            eng.Qb.copy_(torch.from_numpy(Qb).to(eng.dev))
            eng.stop_iter.copy_(torch.tensor(STOPS, dtype=torch.int32).to(eng.dev))
            torch.cuda.synchronize()
            for k, stop in enumerate(STOPS):
                tt = stop if stop != 0 and stop < t else t
                plane = S[(tt - 1) & 1, k]
                row, want_map = PL.host_policy_record(Tab[k], plane & 1, (plane >> 4) & 1, BINS, edges)
                other = PL.host_policy_record(Tab[k], S[tt & 1, k] & 1, (S[tt & 1, k] >> 4) & 1, BINS, edges)[0]
                assert not np.array_equal(row, other), k        # the two planes tell apart
                rec = eng.policy_record(k, BINS, RANGE)
                got = np.concatenate([rec["counts"].ravel(), rec["bonds"], rec["gap_hist"].ravel()])
                assert np.array_equal(got, row), (t, k, tt, got.tolist(), row.tolist())
                assert np.array_equal(eng.policy_map(k), want_map), (t, k, tt)
    finally:
        eng.close()


ABSORBING = dict(R.BASE, alg_alpha=None, alg_gamma=None, epsilon=0.0, epsilon_min=0.0)


def test_a_replica_that_absorbs_mid_run(monkeypatch):
    """Replicas that really absorb (never exploring, at C and at D), in a group of their own that the
    engine retires mid-run, beside a group that keeps running: recorded before, at and after s."""
    _force(monkeypatch)
    over = [dict(reward_weight_payoff=1.0, r=2.0, cost=4), dict(reward_weight_payoff=0.0),
            dict(reward_weight_payoff=1.0, r=0.3), dict(reward_weight_payoff=0.7)]
    rows = [dict(ABSORBING, **o) for o in over] + P.B_ROWS["dyadic"][:4]
    b = P.Batch("absorbing", "philox", 5, 16, True, "reputation", "qlearning", rows, tuple(range(800, 808)))   # T = 16: four turns after the last stop
    exp = PO.expected(b)
    stops = [e.stop_iter for e in exp]
    assert all(1 < s < 12 for s in stops[:4]) and not any(stops[4:]), stops
    ends = [(int(np.all(e.final["S"] == 1)), e.stop_iter & 1) for e in exp[:4]]      # (at D, odd)
    assert sorted(ends) == [(0, 0), (0, 1), (1, 0), (1, 1)], (ends, stops)
    _run(b, absorbing=True, guard=False, streams=2)
    eng = _engine(b, streams=2)
    try:
        eng.run(chunk=2, snapshots=False, policy_every=1, policy_bins=BINS, policy_gap_range=RANGE)
        assert not eng.groups[0]["live"] and eng.groups[1]["live"]
        _check_history(eng, exp)
    finally:
        eng.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_errors(monkeypatch):
    _force(monkeypatch)
    b = _short(P.batch_b("dyadic", "qlearning", True, "reputation", "philox"), reps=2)
    eng = _engine(b)
    try:
        lib, ctx = eng.lib, eng.ctx
        w = PL.policy_width(BINS)
        out = torch.zeros((2, w), dtype=torch.int32, device=eng.dev)
        edges, plane = eng._policy_edges(BINS, (-RANGE, RANGE)), eng._policy_plane()
        call = lambda t, bins=BINS, e=edges.data_ptr(), p=plane.data_ptr(), o=out.data_ptr(), stride=w: lib.spgg_policy(  # noqa: E731
            ctx, t, bins, e, p, o, stride, eng.stream)
        assert call(1) == _lib.OK
        assert call(2) == _lib.E_STATE and b"spgg_policy" in lib.spgg_last_error(ctx)
        eng.step(3)
        assert call(4) == _lib.OK
        for t in (1, 3, 5):
            assert call(t) == _lib.E_STATE, t
        assert call(0) == _lib.E_ARG
        for bins in (0, 257):
            assert call(4, bins=bins) == _lib.E_ARG, bins
        assert call(4, e=None) == _lib.E_ARG and call(4, p=None) == _lib.E_ARG and call(4, o=None) == _lib.E_ARG
        assert call(4, stride=w - 1) == _lib.E_ARG
        eng.flush()
        assert call(4) == _lib.OK and call(3) == _lib.E_STATE
        torch.cuda.synchronize()
        for kw in (dict(policy_every=-1), dict(policy_every=2, policy_bins=0), dict(policy_every=2, policy_bins=257),
                   dict(policy_every=2, policy_gap_range=0.0), dict(policy_every=2, policy_gap_range=(1.0, 1.0)),
                   dict(policy_every=2, policy_gap_range=float("nan"))):
            with pytest.raises(ValueError):
                eng.run(snapshots=False, **kw)
        assert eng._policy_work is plane and "policy" not in eng.records
        with pytest.raises(ValueError):
            eng.policy_histories()
        with pytest.raises(ValueError):
            eng.policy_record(0, bins=300)
    finally:
        eng.close()
    # before bind / set_params
    ctx = ctypes.c_void_p()
    cfg = _lib.Config(device=0, n_rep=1, L=8, second_order=0, state_mode=0, rng_mode=_lib.RNG_PHILOX, iterations=4,
                      rep_int8=0, algorithm=0, batch_reps=1)
    lib = _lib.load()
    _lib.check(lib.spgg_create(ctypes.byref(ctx), cfg), None, "spgg_create")
    try:
        assert lib.spgg_policy(ctx, 1, 4, 8, 8, 8, 64, None) == _lib.E_STATE
    finally:
        lib.spgg_destroy(ctx)


def test_persistent_engine_refuses(monkeypatch):
    _force(monkeypatch, SPGG_PERSIST="1", SPGG_APT="2")
    eng = _engine(P.batch_f(60))
    try:
        assert eng.persistent
        with pytest.raises(ValueError):
            eng.run(snapshots=False, policy_every=2)
        with pytest.raises(ValueError):
            eng.policy_record(0)
        with pytest.raises(ValueError):
            eng.policy_map(0)
        assert eng.t == 1 and eng._policy_work is None
        out = torch.zeros((len(eng.reps), PL.policy_width(4)), dtype=torch.int32, device=eng.dev)
        plane = torch.zeros((len(eng.reps), eng.n), dtype=torch.uint8, device=eng.dev)
        e = torch.zeros((len(eng.reps), 5), dtype=torch.float64, device=eng.dev)
        assert eng.lib.spgg_policy(eng.ctx, 1, 4, e.data_ptr(), plane.data_ptr(), out.data_ptr(), out.shape[1],
                                   eng.stream) == _lib.E_STATE
    finally:
        eng.close()


# ---- the drop-in and the sweep ---------------------------------------------------------------------------------------------
def test_dropin_writes_the_datasets(tmp_path):
    L, T, bins = 16, 20, 6
    m = spgg_amd.SPGG(L=L, iterations=T, r=3.0, use_second_order=True)
    m.save_png = False
    m.policy_history_every, m.policy_history_bins, m.policy_history_gap_range, m.policy_map_final = 4, bins, 0.25, True
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    assert len(ds["coop_rate_history"]) == T
    its = np.arange(1, T + 1, 4)
    assert np.array_equal(ds["policy_history_iters"], its)
    shapes = dict(policy_count_history=(len(its), 4, 2, 2), policy_bond_history=(len(its), 5),
                  policy_gap_hist_history=(len(its), 2, 2, bins + 2))
    for name, shape in shapes.items():
        assert ds[name].shape == shape and ds[name].dtype == np.int64, name
    assert np.array_equal(ds["policy_gap_bin_edges"], PL.policy_bin_edges(0.25, bins))
    nc = np.rint(ds["coop_rate_history"] * L * L).astype(np.int64)
    assert np.array_equal(ds["policy_count_history"][:, :, 0].sum(axis=(1, 2)), nc[its - 1])
    assert np.all(ds["policy_count_history"].sum(axis=(1, 2, 3)) == L * L)
    assert np.all(ds["policy_bond_history"].sum(axis=1) == 2 * L * L)
    assert np.array_equal(ds["policy_gap_hist_history"][:, 0].sum(axis=2), np.stack([nc[its - 1]] * 2, axis=1))
    # the final map: the host model on the state the drop-in is left in
    p = O.Params(L=L, use_second_order=True, state_representation="reputation")
    _row, plane = PL.host_policy_record(m.q_table, m._Sn, O.get_state(m._Sn, m.R, p), bins, PL.policy_bin_edges(0.25, bins))
    assert ds["policy_map_final"].dtype == np.uint8 and np.array_equal(ds["policy_map_final"], plane)

    m2 = spgg_amd.SPGG(L=L, iterations=T, r=3.0)      # the defaults: no dataset of the record
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    extra = set(PL.POLICY_DATASETS) | {PL.POLICY_MAP_DATASET}
    assert not extra & set(read_datasets(fn2)) and extra <= set(ds)


def test_sweep_carries_the_options(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    combos = [(3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning"), (4.0, 0.5, False, 0.8, 0.9, 1.0, "reputation", "qlearning")]
    opts = dict(policy_history_every=3, policy_history_bins=5, policy_history_gap_range=0.3)
    SW.run_batch(combos, seeds=[1, 2], save_png=False, verbose=False, L=16, iterations=14, policy_map_final=True, **opts)
    kw = dict(SW.RUNNER_MODEL, L=16, iterations=14)
    reps = [SW._replica(SW.unpack(p), kw, s) for p, s in zip(combos, (1, 2))]
    init = [reference_init(16, np.random.RandomState(s), algorithm="qlearning") for s in (1, 2)]
    eng = BatchEngine(16, 14, reps, use_second_order=False, state_representation="reputation", rng="mt19937", init=init)
    try:
        eng.run(policy_every=3, policy_bins=5, policy_gap_range=0.3)
        hist = eng.policy_histories()
        maps = [eng.policy_map(k) for k in range(2)]
    finally:
        eng.close()
    for k, p in enumerate(combos):
        got = read_datasets(str(tmp_path / SW.get_folder_name(*SW.unpack(p)) / "data" / "experiment_data.h5"))
        for name in PL.POLICY_DATASETS:
            assert np.array_equal(got[name], hist[k][name]), (k, name)
        assert np.array_equal(got["policy_map_final"], maps[k]), k
        assert got["policy_history_iters"].tolist() == list(range(1, len(got["coop_rate_history"]) + 1, 3))
