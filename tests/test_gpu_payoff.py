"""The payoff record on the device (spgg_payoff_census / spgg_payoff_pairs; BatchEngine.run(payoff_every=),
payoff_census, payoff_pair_sums, payoff_map) against the host model (spgg_amd.payoff: np.roll) on
synthetic planes and on the oracle's S_t.  Integers, exact; no expectation comes from the device.  The
shapes are the smallest at which each part can go wrong: sides the stencil wraps onto itself at, an odd
side, sides no tile divides, the thresholds between the pair-sum instances."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib, payoff as PF, sweep as SW  # noqa: E402
from spgg_amd.engine import BatchEngine, InitState  # noqa: E402
from spgg_amd.h5io import h5native, read_datasets  # noqa: E402
from tests import _observers as OB  # noqa: E402
from tests import _params as P  # noqa: E402
from tests import _payoff as K  # noqa: E402
from tests import _record as R  # noqa: E402
from tests.test_gpu_clusters import _params  # noqa: E402
from tests.test_gpu_record import _force  # noqa: E402


def _plane_engine(L, count, T=4):
    init = [InitState(Q=np.zeros((L, L, 2, 2)), S=np.zeros((L, L), dtype=np.int64)) for _ in range(count)]
    return BatchEngine(L, T, [_params(seed=k) for k in range(count)], use_second_order=False, rng="philox", init=init)


def _set_planes(eng, planes, buf=0):
    """The replicas' S planes (bookkeeping bits too) as the state of an iteration that lies in plane `buf`."""
    torch.cuda.synchronize()
    eng.S[buf].copy_(torch.from_numpy(np.stack([s.reshape(-1) for s in planes])).to(eng.dev))
    torch.cuda.synchronize()
    eng._final_cache = {}


# ---- synthetic planes: census, bonds, plane -------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 4, 5, 13, 18, 37, 200])
def test_census_of_synthetic_planes(L):
    """3, 4, 5: the stencil wraps onto itself; 13: odd, replica planes at odd byte offsets; 37: two tiles
    across and five down, none dividing; 200: seven tiles across.  Three replicas (the last round: two)
    hold different lattices, every byte with random bookkeeping bits."""
    pats = K.patterns(L)
    names = list(pats)
    eng = {3: _plane_engine(L, 3), 2: _plane_engine(L, 2)}
    try:
        for i in range(0, len(names), 3):
            group = names[i:i + 3]
            e = eng[len(group)]
            planes = [K.dirty(pats[name], 100 * L + i + j) for j, name in enumerate(group)]
            assert all(np.any(p >> 1) for p in planes)
            _set_planes(e, planes)
            null = torch.zeros((len(group), K.SLOTS), dtype=torch.int32, device=e.dev)
            e._observe(e.lib.spgg_payoff_census, 1, (None,), null)          # without a plane: the same row
            for k, name in enumerate(group):
                want, want_plane = PF.host_payoff_census(pats[name])
                got = e.payoff_census(k)
                assert got.dtype == np.int64 and got.shape == (K.SLOTS,)
                assert np.array_equal(got, want), (L, name, np.nonzero(got != want)[0].tolist(), got[got != want], want[got != want])
                m = e.payoff_map(k)
                assert m.dtype == np.uint8 and np.array_equal(m, want_plane), (L, name)
                assert np.array_equal(null[k].cpu().numpy(), want), (L, name, "null plane")
    finally:
        for e in eng.values():
            e.close()


# ---- pair sums ----------------------------------------------------------------------------------------------------------
def _pair_planes(L):
    rs = np.random.RandomState(4000 + L)
    a = (rs.rand(L, L) < 0.4).astype(np.int64)
    a[:, -3:] = 0                 # cooperators across the wrap
    a[-2:, :] = 1
    b = K.patterns(L)["checkerboard"] if L < 64 else (rs.rand(L, L) < 0.7).astype(np.int64)
    return [a, b]


@pytest.mark.parametrize("L", [5, 13, 37, 256, 257, 404, 405])
def test_pair_sums(L):
    """256 / 257: the last side of the LDS instance that shares a CU and the first of the one that takes it
    whole; 404 / 405: the last side staged in LDS and the first read from global memory.  max_d = L // 2
    and one smaller value; two replicas with different lattices."""
    strategies = _pair_planes(L)
    D = L // 2
    eng = _plane_engine(L, 2)
    try:
        assert eng.payoff_pairs_max_side == K.max_side()
        _set_planes(eng, [K.dirty(s, L + k) for k, s in enumerate(strategies)])
        for k, S in enumerate(strategies):
            want = PF.host_payoff_pairs(S, D)
            got = eng.payoff_pair_sums(k)
            assert got.dtype == np.int64 and got.shape == (PF.pairs_width(D),)
            assert np.array_equal(got, want), (L, k, np.nonzero(got != want)[0].tolist()[:12])
            d = max(0, min(3, D - 1))
            sK, sc, rows, cols = PF.split_pairs(want, D)
            small = np.concatenate([[sK, sc], rows[:d + 1].ravel(), cols[:d + 1].ravel()])
            assert np.array_equal(eng.payoff_pair_sums(k, d), small), (L, k, d)
            pc = eng.pair_counts(k, d) if L <= eng.correlations_max_side else None
            assert pc is None or (np.array_equal(rows[:d + 1, 2], pc[0]) and np.array_equal(cols[:d + 1, 2], pc[1]))
    finally:
        eng.close()


# ---- the plane rule -----------------------------------------------------------------------------------------------------
STOPS = (0, 3, 4, 6)     # live; absorbed at an odd, at an even iteration; at the first observed one
TIMES = (6, 7)


def test_absorbed_replicas_read_the_plane_of_their_absorbing_iteration():
    """tests/test_gpu_observed_plane.py's rule for this observer: every replica holds two different
    lattices; the record of t is that of plane (tt - 1) & 1, tt = s for a replica absorbed at s < t."""
    L, Rn = 5, len(STOPS)
    rs = np.random.RandomState(41)
    S = ((rs.rand(2, Rn, L, L) < 0.45).astype(np.uint8) | (rs.randint(0, 16, (2, Rn, L, L)) << 1)).astype(np.uint8)
    eng = _plane_engine(L, Rn, T=8)
    try:
        torch.cuda.synchronize()
        eng.S.copy_(torch.from_numpy(S.reshape(2, Rn, L * L)).to(eng.dev))
        eng.stop_iter.copy_(torch.tensor(STOPS, dtype=torch.int32).to(eng.dev))
        torch.cuda.synchronize()
        D = L // 2
        plane = eng._payoff_plane()
        for t in TIMES:
            row = torch.zeros((Rn, K.SLOTS), dtype=torch.int32, device=eng.dev)
            pairs = torch.zeros((Rn, PF.pairs_width(D)), dtype=torch.int64, device=eng.dev)
            eng._observe(eng.lib.spgg_payoff_census, t, (plane,), row)
            eng._observe(eng.lib.spgg_payoff_pairs, t, (D, plane), pairs)
            torch.cuda.synchronize()
            for k, stop in enumerate(STOPS):
                tt = stop if stop != 0 and stop < t else t
                p = (tt - 1) & 1
                want, want_plane = PF.host_payoff_census(S[p, k])
                other = PF.host_payoff_census(S[1 - p, k])[0]
                assert not np.array_equal(want, other), k               # the two planes tell apart
                assert np.array_equal(row[k].cpu().numpy(), want), (t, k, tt)
                assert np.array_equal(plane[k].cpu().numpy().reshape(L, L), want_plane), (t, k, tt)
                assert np.array_equal(pairs[k].cpu().numpy(), PF.host_payoff_pairs(S[p, k], D)), (t, k, tt)
    finally:
        eng.close()


# ---- the in-run record ------------------------------------------------------------------------------------------------------
ABSORBING = dict(R.BASE, alg_alpha=None, alg_gamma=None, epsilon=0.0, epsilon_min=0.0)
EVERY, MAX_D = 3, 4


def _batch(rng):
    """L = 18, three replicas: one that runs on, one that absorbs at t = 6 (between two recorded
    iterations), one that absorbs at t = 16 (a recorded one)."""
    rows = [P.B_ROWS["dyadic"][0], dict(ABSORBING, reward_weight_payoff=0.0), dict(ABSORBING, reward_weight_payoff=1.0, r=2.0, cost=4)]
    return P.Batch("payoff", rng, 18, 20, True, "reputation", "qlearning", rows, (900, 902, 901))


def _engine(b, **kw):
    reps = [P.replica_params(row, s) for row, s in zip(b.rows, b.seeds)]
    return BatchEngine(b.L, b.T, reps, use_second_order=b.M2, state_representation=b.state, rng=b.rng, algorithm=b.alg, **kw)


def _check_final(eng, exp):
    for k, e in enumerate(exp):
        S = e.S[e.t_final]
        want, want_plane = PF.host_payoff_census(S)
        assert np.array_equal(eng.payoff_census(k), want), k
        assert np.array_equal(eng.payoff_map(k), want_plane), k
        assert np.array_equal(eng.payoff_pair_sums(k, MAX_D), PF.host_payoff_pairs(S, MAX_D)), k


@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("rng", ["mt19937", "philox"])
def test_in_run_record(rng, streams, monkeypatch):
    _force(monkeypatch)
    b = _batch(rng)
    exp = OB.expected(b)
    assert [e.stop_iter for e in exp] == [0, 6, 16]
    assert any(not np.array_equal(K.datasets(exp[0], 1, None)["payoff_census_history"][t], K.datasets(exp[0], 1, None)[
        "payoff_census_history"][t - 1]) for t in (3, 6, 9))          # a record of S_{t-1} would not pass
    eng = _engine(b, streams=streams)
    try:
        assert eng.G == streams and not eng.persistent
        eng.run(snapshots=False, payoff_every=EVERY, payoff_max_d=MAX_D)
        hist = eng.payoff_histories()
        for k, e in enumerate(exp):
            K.compare(hist[k], K.datasets(e, EVERY, MAX_D), k)
        assert [len(h["payoff_history_iters"]) for h in hist] == [7, 2, 6]
        OB.assert_run(eng, exp)                   # the run itself is the oracle's: the record does not disturb it
        _check_final(eng, exp)
    finally:
        eng.close()


def test_continued_with_the_same_and_with_other_settings(monkeypatch):
    """run() goes to the engine's last iteration, so a run is continued as the other records' tests
    continue it: started at a later iteration after plain steps, and asked for again."""
    _force(monkeypatch)
    b = _batch("philox")
    exp = OB.expected(b)
    T0 = 5
    eng = _engine(b)
    try:
        eng.step(T0 - 1)
        eng.run(snapshots=False, payoff_every=EVERY, payoff_max_d=MAX_D)       # recorded from t0 = 5 on
        rec, outs = eng.records["payoff"], list(eng.records["payoff"].out)
        assert rec.t0 == T0 and rec.key == (EVERY, MAX_D)
        assert [tuple(o.shape) for o in outs] == [(3, (b.T - T0) // EVERY + 1, K.SLOTS), (3, (b.T - T0) // EVERY + 1, PF.pairs_width(MAX_D))]
        first = eng.payoff_histories()
        for k, e in enumerate(exp):
            K.compare(first[k], K.datasets(e, EVERY, MAX_D, t0=T0), k)
        eng.run(snapshots=False, payoff_every=EVERY, payoff_max_d=MAX_D)       # the same settings: the same record
        assert eng.records["payoff"] is rec and all(x is y for x, y in zip(rec.out, outs))
        for x, y in zip(first, eng.payoff_histories()):
            assert all(np.array_equal(x[key], y[key]) for key in x)
        OB.assert_run(eng, exp)
        _check_final(eng, exp)
        eng.run(snapshots=False, payoff_every=2)                               # other settings: afresh at the current t
        other = eng.records["payoff"]
        assert other is not rec and other.t0 == eng.t == b.T + 1 and other.key == (2, None) and len(other.out) == 1
        for h in eng.payoff_histories():
            assert len(h["payoff_history_iters"]) == 0 and "payoff_pair_sums_history" not in h
        eng.run(snapshots=False)                                               # nothing asked: the record stays readable
        assert eng.records["payoff"] is other
    finally:
        eng.close()


def test_persistent_context(monkeypatch):
    """A function of S_t alone: allowed on a context that steps in persistent launches, at its launch
    boundaries (the record's turns)."""
    monkeypatch.setenv("SPGG_TUNING", "1")
    _force(monkeypatch, SPGG_PERSIST="1", SPGG_APT="2")
    b = P.batch_f(60)
    b = b._replace(rows=b.rows[:3], seeds=b.seeds[:3])
    exp = OB.expected(b)
    eng = _engine(b)
    try:
        assert eng.persistent
        eng.run(chunk=5, snapshots=False, payoff_every=EVERY, payoff_max_d=MAX_D)
        hist = eng.payoff_histories()
        for k, e in enumerate(exp):
            K.compare(hist[k], K.datasets(e, EVERY, MAX_D), k)
        OB.assert_run(eng, exp)
        _check_final(eng, exp)
    finally:
        eng.close()


# ---- the drop-in and the sweep ----------------------------------------------------------------------------------------------
def _check_file(ds, L, every, D, with_map):
    its = np.arange(1, len(ds["coop_rate_history"]) + 1, every)
    assert np.array_equal(ds["payoff_history_iters"], its) and ds["payoff_history_iters"].dtype == np.int64
    assert ds["payoff_census_history"].shape == (len(its), 2, 5, 26) and ds["payoff_census_history"].dtype == np.int64
    assert ds["payoff_bond_history"].shape == (len(its), 103) and ds["payoff_bond_history"].dtype == np.int64
    assert ds["payoff_values"].shape == (2, 26) and ds["payoff_values"].dtype == np.float64
    assert (D is not None) == ("payoff_pair_sums_history" in ds) and with_map == ("payoff_map_final" in ds)
    assert its[0] == 1 and its[3] == 10           # the rows of the reference's snapshot iterations 1 and 10
    for row, i in ((0, 1), (3, 10)):
        want = PF.host_payoff_census(ds[f"Sn_snapshot_{i}"])[0]
        got = np.concatenate([ds["payoff_census_history"][row].ravel(), ds["payoff_bond_history"][row]])
        assert np.array_equal(got, want), i
        if D is not None:
            assert np.array_equal(ds["payoff_pair_sums_history"][row], PF.host_payoff_pairs(ds[f"Sn_snapshot_{i}"], D)), i
    nc = np.rint(ds["coop_rate_history"] * L * L).astype(np.int64)
    assert np.array_equal(ds["payoff_census_history"][:, 0].sum(axis=(1, 2)), nc[its - 1])
    if with_map:
        assert ds["payoff_map_final"].dtype == np.uint8
        assert np.array_equal(ds["payoff_map_final"], PF.host_payoff_census(ds["Sn_final"])[1])


SINKS = ("npz",) + (("native",) if h5native.available() else ())


@pytest.mark.parametrize("sink", SINKS)
def test_dropin_writes_the_datasets(sink, tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", sink)
    L, T = 16, 20
    m = spgg_amd.SPGG(L=L, iterations=T, r=3.0, use_second_order=True)
    m.save_png = False
    m.payoff_history_every, m.payoff_max_distance, m.payoff_map_final = 3, 4, True
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    assert len(ds["coop_rate_history"]) == T
    _check_file(ds, L, 3, 4, True)
    assert np.array_equal(ds["payoff_values"], PF.payoff_values(dict(r=3.0, c=1, cost=0.5)))

    m2 = spgg_amd.SPGG(L=L, iterations=T, r=3.0, use_second_order=True)      # the defaults: the file of before
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    plain = read_datasets(fn2)
    extra = set(PF.PAYOFF_DATASETS) | {PF.PAYOFF_PAIRS_DATASET, PF.PAYOFF_MAP_DATASET}
    assert not extra & set(plain) and set(ds) - set(plain) == extra and set(plain) <= set(ds)


@pytest.mark.parametrize("sink", SINKS)
def test_sweep_carries_the_options(sink, tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", sink)
    monkeypatch.chdir(tmp_path)
    combos = [(3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning"), (4.0, 0.5, False, 0.8, 0.9, 1.0, "reputation", "qlearning")]
    SW.run_batch(combos, seeds=[1, 2], save_png=False, verbose=False, L=16, iterations=14, payoff_history_every=3,
                 payoff_map_final=True)
    for p in combos:
        got = read_datasets(str(tmp_path / SW.get_folder_name(*SW.unpack(p)) / "data" / "experiment_data.h5"))
        _check_file(got, 16, 3, None, True)
        assert np.array_equal(got["payoff_values"], PF.payoff_values(dict(r=p[0], c=SW.RUNNER_MODEL["c"], cost=SW.RUNNER_MODEL["cost"])))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_errors(monkeypatch):
    _force(monkeypatch)
    L = 10
    eng = _plane_engine(L, 2)
    try:
        lib, ctx = eng.lib, eng.ctx
        D = L // 2
        w = PF.pairs_width(D)
        row = torch.zeros((2, K.SLOTS), dtype=torch.int32, device=eng.dev)
        pairs = torch.zeros((2, w), dtype=torch.int64, device=eng.dev)
        plane = torch.full((2, L * L), 255, dtype=torch.uint8, device=eng.dev)
        census = lambda t=1, p=plane.data_ptr(), o=row.data_ptr(), stride=K.SLOTS: lib.spgg_payoff_census(  # noqa: E731
            ctx, t, p, o, stride, eng.stream)
        pair = lambda t=1, d=D, p=plane.data_ptr(), o=pairs.data_ptr(), stride=w: lib.spgg_payoff_pairs(  # noqa: E731
            ctx, t, d, p, o, stride, eng.stream)
        assert census(t=0) == _lib.E_ARG and b"spgg_payoff_census" in lib.spgg_last_error(ctx)
        assert census(o=None) == _lib.E_ARG and census(stride=K.SLOTS - 1) == _lib.E_ARG
        assert pair(t=0) == _lib.E_ARG and pair(d=-1) == _lib.E_ARG and pair(d=D + 1) == _lib.E_ARG
        assert b"L / 2" in lib.spgg_last_error(ctx)
        assert pair(o=None) == _lib.E_ARG and pair(stride=w - 1) == _lib.E_ARG
        assert pair(p=None) == _lib.E_ARG and b"plane" in lib.spgg_last_error(ctx)
        torch.cuda.synchronize()
        assert not row.cpu().numpy().any() and not pairs.cpu().numpy().any() and np.all(plane.cpu().numpy() == 255)   # nothing was enqueued
        for kw in (dict(payoff_every=-1), dict(payoff_every=2, payoff_max_d=D + 1), dict(payoff_every=2, payoff_max_d=-1)):
            with pytest.raises(ValueError):
                eng.run(snapshots=False, **kw)
            assert eng.t == 1
        assert eng._payoff_work is None and "payoff" not in eng.records
        with pytest.raises(ValueError):
            eng.payoff_histories()
        with pytest.raises(ValueError):
            eng.payoff_pair_sums(0, D + 1)
        assert census() == _lib.OK and pair() == _lib.OK
    finally:
        eng.close()
    ctx = ctypes.c_void_p()      # before bind
    cfg = _lib.Config(device=0, n_rep=1, L=8, second_order=0, state_mode=0, rng_mode=_lib.RNG_PHILOX, iterations=4,
                      rep_int8=0, algorithm=0, batch_reps=1)
    lib = _lib.load()
    _lib.check(lib.spgg_create(ctypes.byref(ctx), cfg), None, "spgg_create")
    try:
        assert lib.spgg_payoff_census(ctx, 1, 8, 8, K.SLOTS, None) == _lib.E_STATE
        assert lib.spgg_payoff_pairs(ctx, 1, 0, 8, 8, 8, None) == _lib.E_STATE
    finally:
        lib.spgg_destroy(ctx)
