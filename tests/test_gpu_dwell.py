"""The strategy dwell record on the device (spgg_dwell_*) against the NumPy model written from its
definitions (tests/_dwell.py) on the planes of a plain engine stepped one iteration at a time
(tests/test_gpu_clusters._stepwise_expectation; the steps themselves are pinned to the oracle
elsewhere), against the oracle-pinned history record (stats_folded) and against the oracle's own
planes.  Every comparison of the record is of integers and exact.  "The record does not disturb
the run" is held as tests/test_gpu_clusters.py holds it (its ORDER_DEPENDENT set and SUM_ORDER_TOL,
derived there for the L = 24 case used here)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib, dwell  # noqa: E402
from spgg_amd.engine import BatchEngine, plan_groups, reference_init  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402
from oracle import spgg_oracle as O  # noqa: E402

from tests import _dwell as M  # noqa: E402
from tests.test_gpu_clusters import ORDER_DEPENDENT, SUM_ORDER_TOL, _params, _stepwise_expectation  # noqa: E402


def _make_l24(T=40):
    def make():
        seeds = (11, 12, 13)
        reps = [_params(seed=s) for s in seeds]
        init = [reference_init(24, np.random.RandomState(s), S_in_one=np.zeros((24, 24), dtype=int) if k == 1 else None)
                for k, s in enumerate(seeds)]   # replica 1 starts all-C: absorbed at t = 1
        return BatchEngine(24, T, reps, use_second_order=True, state_representation="action", rng="mt19937", init=init)
    return make


def _make_philox(L, T, R=3, M2=False):
    return lambda: BatchEngine(L, T, [_params(seed=40 + L + k) for k in range(R)], use_second_order=M2, rng="philox")


def _with_final(eng, planes, last):
    """planes[k] with the state after the last executed iteration added (S_{T+1} of a replica that
    ran to the end: final_state's), and the state index of that final state."""
    out, t_final = [], []
    for k in range(eng.R):
        p = dict(planes[k])
        if not int(eng.stopped[k]):
            p[last[k] + 1] = eng.final_state(k)[2]
        out.append(p)
        t_final.append(last[k] if int(eng.stopped[k]) else last[k] + 1)
    return out, t_final


def _assert_histories(hist, planes, last, every, t_ref=1):
    for k, h in enumerate(hist):
        its = np.arange(t_ref, last[k] + 1, every)
        assert tuple(h) == dwell.DWELL_DATASETS
        assert np.array_equal(h["dwell_history_iters"], its) and h["dwell_ref_iteration"] == t_ref, k
        want = np.array([M.of_replica(planes[k], last[k], t_ref, t)[0] for t in its], dtype=np.int64).reshape(-1, M.SLOTS)
        got = np.concatenate([h["persistence_history"], h["autocorrelation_history"], h["flip_total_history"][:, None],
                              h["cooperator_time_history"][:, None], h["strategy_age_hist_history"].reshape(len(its), -1)],
                             axis=1)
        assert got.dtype == np.int64 and got.shape == want.shape, (k, got.shape)
        assert np.array_equal(got, want), (k, every, np.argwhere(got != want)[:5])


def _assert_final(eng, planes, last, t_ref=1):
    """dwell_record() and dwell_fields(k) after a run: those of the state final_state returns."""
    full, t_final = _with_final(eng, planes, last)
    rows = eng.dwell_record()
    assert rows.dtype == np.int64 and rows.shape == (eng.R, 61)
    for k in range(eng.R):
        want_row, want_f = M.of_replica(full[k], t_final[k], t_ref, t_final[k])
        assert np.array_equal(rows[k], want_row), (k, np.argwhere(rows[k] != want_row).ravel())
        f = eng.dwell_fields(k)
        assert sorted(f) == ["cooperation_frequency", "flip_count", "strategy_age"]
        for key, w in zip(("flip_count", "strategy_age"), want_f):
            assert f[key].shape == (eng.L, eng.L) and np.array_equal(f[key].ravel(), w), (k, key)
        freq = f["cooperation_frequency"]
        assert freq.dtype == np.float64 and np.array_equal(freq.ravel(), want_f[2] / np.float64(max(t_final[k], t_ref) - t_ref + 1))


# L = 24: the other records' setup (one replica absorbed at t = 1); L = 13: n odd, the byte path and
# unaligned replica bases; L = 18: n % 4 == 0 but n % 16 != 0, the dword path with a tail
@pytest.mark.parametrize("every", [1, 7])
@pytest.mark.parametrize("case", ["L24", "L13", "L18"])
def test_rows_and_fields_against_the_model(case, every, expectations):
    T = 40
    make = _make_l24(T) if case == "L24" else _make_philox(int(case[1:]), T)
    planes, last = expectations(case, make, T)
    if case == "L24":
        assert last[1] == 1 and last[0] > 7
    eng = make()
    try:
        assert eng.n % 4 == {"L24": 0, "L13": 1, "L18": 0}[case] and (case != "L18" or eng.n % 16)
        eng.run(snapshots=False, dwell_every=every)
        assert [eng.last_iteration(k) for k in range(eng.R)] == last
        assert eng.records["dwell"].out[0].shape[1] == (T - 1) // every + 1
        _assert_histories(eng.dwell_histories(), planes, last, every)
        _assert_final(eng, planes, last)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def expectations():
    """The stepwise planes of a case, computed once per module and left unchanged."""
    cache = {}

    def get(name, make, T):
        if name not in cache:
            cache[name] = _stepwise_expectation(make, T)
        return cache[name]
    return get


def test_a_replica_that_absorbs_mid_run(expectations):
    """The parameters of the golden case m1_rep_L24_stopD (r = 1: defection takes over)."""
    L, T, every = 24, 650, 16

    def make():
        reps = [_params(r=1.0, seed=2), _params(r=3.0, seed=3)]
        return BatchEngine(L, T, reps, use_second_order=False, state_representation="reputation", rng="mt19937")

    planes, last = expectations("stopD", make, T)
    assert 5 < last[0] < T and last[1] == T, last
    eng = make()
    try:
        eng.run(snapshots=False, dwell_every=every)
        hist = eng.dwell_histories()
        assert hist[0]["dwell_history_iters"][-1] == 1 + (last[0] - 1) // every * every <= last[0]   # its rows stop at last
        _assert_histories(hist, planes, last, every)
        _assert_final(eng, planes, last)   # replica 0: the read-outs of S_last
        assert eng.dwell_record()[0, M.NCOOP] == 0 and eng.dwell_record()[0, M.SAME] == np.sum(planes[0][1] == 1)
    finally:
        eng.close()


def test_against_the_history_record(expectations):
    """Independent of the model: NCOOP, FLIPS and COOP_TIME from the oracle-pinned device record."""
    T = 40
    make = _make_l24(T)
    eng = make()
    try:
        eng.run(snapshots=False, dwell_every=1)
        hist = eng.dwell_histories()
        st = eng.stats_folded().cpu().numpy()
        for k in range(eng.R):
            its = hist[k]["dwell_history_iters"]
            nc = st[k, :, _lib.ST_NCOOP].astype(np.int64)
            sw = (st[k, :, _lib.ST_SW_CD] + st[k, :, _lib.ST_SW_DC]).astype(np.int64)
            assert np.array_equal(hist[k]["autocorrelation_history"][:, 2], nc[its]), k
            assert np.array_equal(hist[k]["flip_total_history"], [sw[1:t].sum() for t in its]), k
            assert np.array_equal(hist[k]["cooperator_time_history"], [nc[1:t + 1].sum() for t in its]), k
    finally:
        eng.close()


def test_against_the_oracle():
    L, T, seed, every = 16, 30, 5, 3
    p = _params(seed=seed)
    op = O.Params(L=L, iterations=T, use_second_order=False, state_representation="reputation",
                  **{k: getattr(p, k) for k in ("r", "c", "cost", "alpha", "gamma", "epsilon", "epsilon_decay",
                                                 "epsilon_min", "influence_factor", "lambda_epsilon", "delta_R_D",
                                                 "R_min", "R_max", "reward_weight_payoff", "rep_gain_C")})
    rs = np.random.RandomState(seed)   # the draws of reference_init, then draw_step's per iteration (MT19937)
    Q, S = O.init_state(op, rs)
    R, eps = np.zeros((L, L)), op.epsilon
    planes = {1: S.copy()}
    for i in range(1, T + 1):
        assert 0 < np.sum(S == 0) < L * L
        S, R, Q, _ = O.step(S, R, Q, eps, O.draw_step(rs, L), p=op)
        eps = max(eps * op.epsilon_decay, op.epsilon_min)
        planes[i + 1] = S.copy()
    eng = BatchEngine(L, T, [p], use_second_order=False, state_representation="reputation", rng="mt19937")
    try:
        eng.run(snapshots=False, dwell_every=every)
        assert eng.last_iteration(0) == T and np.array_equal(eng.final_state(0)[2], planes[T + 1])
        _assert_histories(eng.dwell_histories(), [planes], [T], every)
        want_row, want_f = M.of_replica(planes, T + 1, 1, T + 1)
        assert np.array_equal(eng.dwell_record()[0], want_row)
        assert np.array_equal(eng.dwell_fields(0)["flip_count"].ravel(), want_f[0])
    finally:
        eng.close()


def test_replica_groups():
    L, T, every = 200, 10, 3
    R = next(r for r in range(1, 64) if plan_groups(r, L, 1, 1 << 40)[1] >= 2)   # the planner's first split
    make = _make_philox(L, T, R)
    eng = make()
    try:
        assert eng.G >= 2, (R, eng.G)
        eng.run(snapshots=False, dwell_every=every)
        hist = eng.dwell_histories()
        planes, last = _stepwise_expectation(make, T)
        _assert_histories(hist, planes, last, every)   # replicas of every group, through the hook in spgg_step_groups
        _assert_final(eng, planes, last)
    finally:
        eng.close()


def test_ragged_stepping_equals_run():
    L, T = 18, 9
    make = _make_philox(L, T)
    a, b = make(), make()
    try:
        a.dwell_start()
        for k in (3, 1, 5):
            a.step(k)
        b.run(snapshots=False, dwell_every=4)
        assert a.t == b.t == T + 1
        ra, rb = a.dwell_record(), b.dwell_record()
        assert np.array_equal(ra, rb) and ra[:, M.FLIPS].all()
        for k in range(a.R):
            fa, fb = a.dwell_fields(k), b.dwell_fields(k)
            assert all(np.array_equal(fa[key], fb[key]) for key in fa)
    finally:
        a.close()
        b.close()


def test_continuation(expectations):
    """run() goes to the engine's last iteration, so a run is continued as the other records'
    tests continue it: started at a later iteration after plain steps, and asked for again."""
    L, T, T0 = 18, 40, 18
    make = _make_philox(L, T)
    planes, last = expectations("L18", make, T)
    eng = make()
    try:
        eng.step(T0 - 1)
        eng.run(snapshots=False, dwell_every=4)
        rec, out = eng.records["dwell"], eng.records["dwell"].out[0]
        assert rec.t0 == eng.dwell_t_ref == T0 and out.shape == (eng.R, (T - T0) // 4 + 1, 61)
        first = eng.dwell_histories()
        eng.run(snapshots=False, dwell_every=4)   # the same k: one record, one reference
        assert eng.records["dwell"] is rec and rec.out[0] is out and eng.dwell_t_ref == T0
        hist = eng.dwell_histories()
        _assert_histories(hist, planes, last, 4, t_ref=T0)
        for a, b in zip(first, hist):
            assert all(np.array_equal(a[key], b[key]) for key in a)
        _assert_final(eng, planes, last, t_ref=T0)
        eng.run(snapshots=False, dwell_every=5)   # another k: afresh at the current t
        assert eng.records["dwell"] is not rec and eng.dwell_t_ref == eng.t == T + 1
        for k, h in enumerate(eng.dwell_histories()):
            assert h["dwell_ref_iteration"] == T + 1 and len(h["dwell_history_iters"]) == 0
        row = eng.dwell_record()   # the reference is the current state
        assert np.all(row[:, M.NEVER] == eng.n) and np.all(row[:, M.SAME] == eng.n) and not row[:, M.FLIPS].any()
        eng.run(snapshots=False, dwell_every=0)   # 0: disarmed, the record dropped
        assert eng.dwell_t_ref is None and "dwell" not in eng.records
        one = torch.zeros(61, dtype=torch.int64, device=eng.dev)
        assert eng.lib.spgg_dwell_record(eng.ctx, eng.t, one.data_ptr(), 61, eng.stream) == _lib.E_STATE
        with pytest.raises(ValueError):
            eng.dwell_histories()
        with pytest.raises(ValueError):
            eng.dwell_record()
    finally:
        eng.close()


def test_the_record_does_not_disturb_the_run():
    T = 40
    make = _make_l24(T)

    def run(every):
        eng = make()
        try:
            eng.run(snapshots=False, dwell_every=every)
            return dict(final=[eng.final_state(k) for k in range(3)], hist=eng.histories(),
                        mt=[eng.mt_state_host(k) for k in range(3)], last=[eng.last_iteration(k) for k in range(3)])
        finally:
            eng.close()

    plain, got = run(0), run(7)
    assert got["last"] == plain["last"]
    for k in range(3):
        for a, b in zip(got["final"][k], plain["final"][k]):   # Q, R, S
            assert np.array_equal(a, b)
        assert np.array_equal(got["mt"][k][0], plain["mt"][k][0]) and got["mt"][k][1] == plain["mt"][k][1]
        assert set(got["hist"][k]) == set(plain["hist"][k])
        for key, v in plain["hist"][k].items():
            g = got["hist"][k][key]
            if key in ORDER_DEPENDENT:
                assert g.shape == v.shape, (k, key)
                print(key, float(np.nanmax(np.abs(g - v), initial=0.0)))
                np.testing.assert_allclose(g, v, equal_nan=True, err_msg=f"{k} {key}", **SUM_ORDER_TOL)
            else:
                assert np.array_equal(g, v, equal_nan=True), (k, key)


def test_errors():
    L, T = 18, 12
    eng = _make_philox(L, T)()
    try:
        n = eng.n
        rec = torch.zeros(61, dtype=torch.int64, device=eng.dev)
        fld = torch.zeros(3 * n, dtype=torch.int32, device=eng.dev)
        words = torch.zeros((eng.R, n, 3), dtype=torch.int32, device=eng.dev)
        ref = torch.zeros((eng.R, n), dtype=torch.uint8, device=eng.dev)
        lib, ctx, s = eng.lib, eng.ctx, eng.stream
        assert lib.spgg_dwell_reset(ctx, 1, s) == _lib.E_STATE          # nothing bound
        assert lib.spgg_dwell_bind(ctx, words.data_ptr(), None) == _lib.E_ARG
        assert lib.spgg_dwell_bind(ctx, words.data_ptr(), ref.data_ptr()) == _lib.OK
        assert lib.spgg_dwell_record(ctx, 1, rec.data_ptr(), 61, s) == _lib.E_STATE   # bound, not armed
        assert lib.spgg_dwell_fields(ctx, 1, fld.data_ptr(), 3 * n, s) == _lib.E_STATE
        eng.step(4)
        assert lib.spgg_dwell_reset(ctx, 0, s) == _lib.E_ARG
        assert lib.spgg_dwell_reset(ctx, eng.t, s) == _lib.OK          # t_ref = 5
        assert lib.spgg_dwell_record(ctx, 4, rec.data_ptr(), 61, s) == _lib.E_ARG     # t < t_ref
        assert lib.spgg_dwell_fields(ctx, 4, fld.data_ptr(), 3 * n, s) == _lib.E_ARG
        assert lib.spgg_dwell_record(ctx, 5, rec.data_ptr(), 60, s) == _lib.E_ARG     # stride below the row
        assert lib.spgg_dwell_fields(ctx, 5, fld.data_ptr(), 3 * n - 1, s) == _lib.E_ARG
        assert lib.spgg_dwell_record(ctx, 5, None, 61, s) == _lib.E_ARG
        torch.cuda.synchronize()
        assert not rec.cpu().numpy().any() and not fld.cpu().numpy().any()
        assert lib.spgg_dwell_record(ctx, 5, rec.data_ptr(), 61, s) == _lib.OK
        torch.cuda.synchronize()
        row = rec.cpu().numpy()
        assert row[M.NEVER] == row[M.SAME] == n and row[M.FLIPS] == 0 and row[M.AGE0:].sum() == n
        assert lib.spgg_dwell_bind(ctx, None, None) == _lib.OK           # unbinds and disarms
        assert lib.spgg_dwell_record(ctx, 5, rec.data_ptr(), 61, s) == _lib.E_STATE
        assert lib.spgg_dwell_reset(ctx, 5, s) == _lib.E_STATE
        for bad in (-1, -7):
            with pytest.raises(ValueError):
                eng.run(snapshots=False, dwell_every=bad)
            assert eng.dwell_t_ref is None and eng.t == 5   # nothing allocated or enqueued
        torch.cuda.synchronize()
    finally:
        eng.close()


def test_persistent_contexts_refuse(monkeypatch):
    """A context that steps in persistent launches has no launch boundary to hook."""
    monkeypatch.setenv("SPGG_PERSIST", "1")
    eng = BatchEngine(200, 8, [_params(seed=1)], use_second_order=False, rng="philox")
    try:
        if not eng.persistent:
            pytest.skip("this shape does not go persistent here")
        words = torch.zeros((1, eng.n, 3), dtype=torch.int32, device=eng.dev)
        ref = torch.zeros((1, eng.n), dtype=torch.uint8, device=eng.dev)
        assert eng.lib.spgg_dwell_bind(eng.ctx, words.data_ptr(), ref.data_ptr()) == _lib.E_STATE
        with pytest.raises(ValueError):
            eng.run(snapshots=False, dwell_every=2)
        with pytest.raises(ValueError):
            eng.dwell_start()
        assert eng.t == 1
    finally:
        eng.close()


def test_dropin_and_sweep(tmp_path, monkeypatch):
    m = spgg_amd.SPGG(L=16, iterations=30, r=3.0)
    m.save_png = False
    m.dwell_history_every = 5
    m.dwell_fields = True
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    n_it = len(ds["coop_rate_history"])
    assert n_it == 30
    its = np.arange(1, n_it + 1, 5)
    assert np.array_equal(ds["dwell_history_iters"], its) and ds["dwell_ref_iteration"] == 1
    shapes = dict(persistence_history=(len(its), 2), autocorrelation_history=(len(its), 3), flip_total_history=(len(its),),
                  cooperator_time_history=(len(its),), strategy_age_hist_history=(len(its), 2, 27),
                  flip_count_final=(16, 16), strategy_age_final=(16, 16))
    for key, shape in shapes.items():
        assert ds[key].shape == shape and ds[key].dtype == np.int64, key
    # the first row: the initial population; the rest against the datasets of the run itself
    nc = np.rint(ds["coop_rate_history"] * 256).astype(np.int64)   # cooperators of S_1 .. S_30
    sw = ds["switch_C_to_D"] + ds["switch_D_to_C"]                 # flips of the launches 1 .. 30
    assert np.array_equal(ds["autocorrelation_history"][:, 2], nc[its - 1])
    assert np.array_equal(ds["persistence_history"][0], [256, nc[0]])
    assert np.array_equal(ds["flip_total_history"], [sw[:t - 1].sum() for t in its])
    assert np.array_equal(ds["cooperator_time_history"], [nc[:t].sum() for t in its])
    # the final fields are those of S_31 = Sn_final, 31 states after the reference S_1
    coop = ds["cooperation_frequency_final"] * 31
    assert ds["cooperation_frequency_final"].dtype == np.float64 and ds["cooperation_frequency_final"].shape == (16, 16)
    assert np.array_equal(np.rint(coop), coop.round(9)) and np.rint(coop).sum() == nc.sum() + np.sum(ds["Sn_final"] == 0)
    assert np.array_equal(ds["cooperation_frequency_final"], np.rint(coop) / np.float64(31))   # coop / (t - t_ref + 1)
    assert ds["flip_count_final"].sum() == sw.sum()
    assert np.all(ds["strategy_age_final"][ds["flip_count_final"] == 0] == 30)

    m2 = spgg_amd.SPGG(L=16, iterations=30, r=3.0)   # the defaults: today's dataset names
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    plain = read_datasets(fn2)
    extra = set(dwell.DWELL_DATASETS) | set(dwell.DWELL_FIELD_DATASETS)
    assert not extra & set(plain) and set(ds) - set(plain) == extra and set(plain) <= set(ds)

    from spgg_amd import sweep as SW
    monkeypatch.chdir(tmp_path)
    combos = [(3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning"), (4.0, 0.5, False, 0.8, 1.0, 1.0, "reputation", "qlearning")]
    SW.run_batch(combos, seeds=[1, 2], save_png=False, verbose=False, L=16, iterations=20, dwell_history_every=4)
    for p in combos:
        got = read_datasets(str(tmp_path / SW.get_folder_name(*SW.unpack(p)) / "data" / "experiment_data.h5"))
        assert set(dwell.DWELL_DATASETS) <= set(got) and not set(dwell.DWELL_FIELD_DATASETS) & set(got)
        last = len(got["coop_rate_history"])
        assert np.array_equal(got["dwell_history_iters"], np.arange(1, last + 1, 4))
        nc = np.rint(got["coop_rate_history"] * 256).astype(np.int64)
        assert np.array_equal(got["autocorrelation_history"][:, 2], nc[got["dwell_history_iters"] - 1])
