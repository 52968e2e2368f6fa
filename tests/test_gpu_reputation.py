"""Device reputation record (spgg_reputation_hist / spgg_reputation_pairs, ABI v19) against the
host: final values (BatchEngine.reputation_histogram / reputation_pair_sums), the in-run record
(run(reputation_every=k) / reputation_histories), the f64-reputation path, replica groups, the
reference's own rep_hist_* datasets and the drop-in's / sweep's datasets.  Expectations are
np.histogram and np.roll on host copies of S and R (tests/_reputation.py); every comparison is of
integers and exact.  "The record does not disturb the run" is held as tests/test_gpu_clusters.py
holds it: bit identity for the final state, the MT19937 key and every history outside that file's
ORDER_DEPENDENT set, and that file's SUM_ORDER_TOL for the histories the step kernels sum with
atomics, which differ between two identical runs already."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib  # noqa: E402
from spgg_amd.engine import (BatchEngine, InitState, host_reputation_pair_sums, plan_groups,  # noqa: E402
                             reference_init)
from spgg_amd.h5io import read_datasets  # noqa: E402

from tests import _reputation as K  # noqa: E402
from tests._golden import Case  # noqa: E402
from tests.test_gpu_clusters import ORDER_DEPENDENT, SUM_ORDER_TOL, _params  # noqa: E402
from tests.test_gpu_parity import _pinned_model  # noqa: E402

# the two parameter sets: the extreme magnitudes at unit 1, and the default bounds
PARAM_SETS = {"extreme": dict(R_min=-128, R_max=127), "default": dict(R_min=-10, R_max=10)}


def _field_engine(L, fields, planes, **params):
    """An int8-reputation engine whose replicas hold the given S planes and int8 reputation fields
    as (S_1, R_1); nothing is stepped."""
    init = [InitState(Q=np.zeros((L, L, 2, 2)), S=S) for S in planes]
    eng = BatchEngine(L, 4, [_params(seed=k, **params) for k in range(len(planes))], use_second_order=False,
                      rng="philox", init=init)
    assert eng.rep_int8 and np.all(eng.rep_units == 1.0)
    eng.Rep[0].copy_(torch.from_numpy(np.stack([f.reshape(-1) for f in fields])).to(eng.dev))
    eng.S[0].copy_(torch.from_numpy(np.stack([s.reshape(-1) for s in planes])).to(eng.dev))   # bookkeeping bits too
    torch.cuda.synchronize()
    return eng


def _check_engine(eng, fields, planes, names, lo, hi, distances=(None, 0, 1), bins=(20, 256)):
    L = eng.L
    for k, (F, S) in enumerate(zip(fields, planes)):
        for B in bins:
            got = eng.reputation_histogram(k, B)
            assert got.dtype == np.int64 and got.shape == (2, B), (names[k], B)
            assert np.array_equal(got, K.expected_hist(S, F, B, lo, hi)), (names[k], B)
        ws, wr, wc = K.expected_pair_sums(F, L // 2)
        for max_d in distances:
            if max_d is not None and max_d > L // 2:
                continue
            D = L // 2 if max_d is None else max_d
            s, rows, cols = eng.reputation_pair_sums(k, max_d)
            assert rows.dtype == np.int64 and cols.dtype == np.int64 and rows.shape == cols.shape == (D + 1,)
            assert s == ws, (names[k], max_d, s, ws)
            assert np.array_equal(rows, wr[:D + 1]), (names[k], max_d)
            assert np.array_equal(cols, wc[:D + 1]), (names[k], max_d)
            assert rows[0] == cols[0] == int((F.astype(np.int64) ** 2).sum())


def _run_patterns(L, which):
    fields = K.fields_of(L) + [K.fields_of(L, seed=1)[6]]      # + a second random field under dirty S
    names = list(K.FIELD_NAMES) + ["dirty_bits"]
    planes = K.strategy_planes(L, len(fields))                 # odd L: replica planes at odd byte offsets
    p = PARAM_SETS[which]
    eng = _field_engine(L, fields, planes, **p)
    try:
        _check_engine(eng, fields, planes, names, p["R_min"], p["R_max"])
        # custom edges, the same for every replica: a value on the last edge, values outside
        e = np.array([-128.0, -3.0, 0.0, 0.5, 127.0])
        for k in (2, len(fields) - 1):
            x, coop = fields[k].astype(np.float64), (planes[k] & 1) == 0
            want = np.stack([np.histogram(x[coop], bins=e)[0], np.histogram(x[~coop], bins=e)[0]])
            assert np.array_equal(eng.reputation_histogram(k, 4, edges=e), want), k
    finally:
        eng.close()


@pytest.mark.parametrize("which", sorted(PARAM_SETS))
@pytest.mark.parametrize("L", [1, 2, 3, 5, 13, 16, 33, 64])
def test_patterns(L, which):
    _run_patterns(L, which)


def test_patterns_side_200():
    _run_patterns(200, "extreme")


# 405: the smallest side of the instance that reads the plane from global memory, full max_d;
# 1000: cfg5, max_d = 16 so that the host expectation stays cheap
@pytest.mark.parametrize("L,max_d", [(405, None), (1000, 16)])
def test_global_instance(L, max_d):
    rs = np.random.RandomState(L)
    F = rs.randint(-128, 128, (L, L)).astype(np.int8)
    F[:, -7:] = -128          # the extreme magnitude across the wrap
    F[-3:, :] = 127
    S = rs.randint(0, 32, (L, L)).astype(np.uint8)
    eng = _field_engine(L, [F], [S], **PARAM_SETS["extreme"])
    try:
        assert 404 < L <= eng.reputation_max_side == 11520
        _check_engine(eng, [F], [S], [f"random{L}"], -128, 127, distances=(max_d,), bins=(20,))
    finally:
        eng.close()


def test_instance_threshold():
    """256 / 257: the last side of the LDS instance that shares a CU and the first of the one that
    takes it whole; 404: the last side staged in LDS."""
    for L in (256, 257, 404):
        rs = np.random.RandomState(L)
        F = rs.randint(-128, 128, (L, L)).astype(np.int8)
        S = rs.randint(0, 2, (L, L)).astype(np.uint8)
        eng = _field_engine(L, [F], [S], **PARAM_SETS["extreme"])
        try:
            ws, wr, wc = K.expected_pair_sums(F, 9)
            s, rows, cols = eng.reputation_pair_sums(0, 9)
            assert s == ws and np.array_equal(rows, wr) and np.array_equal(cols, wc), L
        finally:
            eng.close()


def test_argument_errors():
    L = 10
    F, S = K.fields_of(L)[6], K.strategy_planes(L, 1)[0]
    eng = _field_engine(L, [F], [S])
    try:
        width = 2 * (L // 2 + 2) + 1
        out = torch.zeros(width, dtype=torch.int64, device=eng.dev)
        pairs, hist = eng.lib.spgg_reputation_pairs, eng.lib.spgg_reputation_hist
        assert pairs(eng.ctx, 0, 1, out.data_ptr(), width, eng.stream) == _lib.E_ARG              # t < 1
        assert pairs(eng.ctx, 1, -1, out.data_ptr(), width, eng.stream) == _lib.E_ARG             # max_d < 0
        assert pairs(eng.ctx, 1, L // 2 + 1, out.data_ptr(), width, eng.stream) == _lib.E_ARG     # max_d > L / 2
        assert "L / 2" in eng.lib.spgg_last_error(eng.ctx).decode()
        assert pairs(eng.ctx, 1, 1, None, width, eng.stream) == _lib.E_ARG                        # null out
        assert pairs(eng.ctx, 1, 1, out.data_ptr(), 4, eng.stream) == _lib.E_ARG                  # rows would overlap
        edges = torch.from_numpy(K.edges_of(-10, 10, 20)).to(eng.dev)
        h = torch.zeros(2 * 300, dtype=torch.int32, device=eng.dev)
        assert hist(eng.ctx, 1, 0, edges.data_ptr(), h.data_ptr(), 600, eng.stream) == _lib.E_ARG    # bins < 1
        assert hist(eng.ctx, 1, 257, edges.data_ptr(), h.data_ptr(), 600, eng.stream) == _lib.E_ARG  # bins > 256
        assert hist(eng.ctx, 1, 20, None, h.data_ptr(), 600, eng.stream) == _lib.E_ARG               # null edges
        assert hist(eng.ctx, 1, 20, edges.data_ptr(), h.data_ptr(), 39, eng.stream) == _lib.E_ARG    # stride < 2 bins
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any() and not h.cpu().numpy().any()
        for bad in (dict(reputation_every=-1), dict(reputation_every=1, reputation_bins=0),
                    dict(reputation_every=1, reputation_bins=257), dict(reputation_every=1, reputation_max_d=L // 2 + 1),
                    dict(reputation_every=1, reputation_max_d=-1)):
            with pytest.raises(ValueError):
                eng.run(snapshots=False, **bad)
            assert eng.t == 1
        with pytest.raises(ValueError):
            eng.reputation_pair_sums(0, L // 2 + 1)
        with pytest.raises(ValueError):
            eng.reputation_histogram(0, 257)
        with pytest.raises(ValueError):
            eng.reputation_histogram(0, 2, edges=[0.0, 1.0, 1.0])
        with pytest.raises(ValueError):
            eng.reputation_histories()
    finally:
        eng.close()


def test_f64_reputation_path():
    """Non-dyadic gains: the reputation buffers hold f64.  The histogram matches np.histogram of the
    host copy; the pair sums are refused by the library, summed on the host by the engine, and
    refused by run() before anything is enqueued."""
    L, T = 24, 12
    reps = [_params(seed=s, rep_gain_C=0.3) for s in (1, 2)]
    eng = BatchEngine(L, T, reps, use_second_order=True, rng="mt19937")
    try:
        assert not eng.rep_int8 and eng.Rep.dtype == torch.float64
        out = torch.zeros(8, dtype=torch.int64, device=eng.dev)
        assert eng.lib.spgg_reputation_pairs(eng.ctx, 1, 1, out.data_ptr(), 8, eng.stream) == _lib.E_ARG
        assert "f64" in eng.lib.spgg_last_error(eng.ctx).decode()
        with pytest.raises(ValueError, match="f64"):
            eng.run(snapshots=False, reputation_every=1, reputation_max_d=2)
        assert eng.t == 1 and "reputation" not in eng.records   # nothing was enqueued
        eng.run(snapshots=False, reputation_every=5, reputation_bins=20)
        assert not out.cpu().numpy().any()
        hist = eng.reputation_histories()
        for k in range(2):
            Q, R, S = eng.final_state(k)
            assert len(np.unique(R)) > 3 and not np.all(R == np.round(R))
            for B in (20, 256):
                assert np.array_equal(eng.reputation_histogram(k, B), K.expected_hist(S, R, B, -10, 10)), (k, B)
            # edges among the values themselves: values on an edge, on the last edge, outside
            e = np.unique(R)[:600:3]
            want = np.stack([np.histogram(R[S == 0], bins=e)[0], np.histogram(R[S == 1], bins=e)[0]])
            assert np.array_equal(eng.reputation_histogram(k, len(e) - 1, edges=e), want), k
            s, rows, cols = eng.reputation_pair_sums(k, 3)
            hs, hr, hc = host_reputation_pair_sums(R, 3)
            assert rows.dtype == np.float64 and s == hs and np.array_equal(rows, hr) and np.array_equal(cols, hc)
            assert set(hist[k]) == {"reputation_history_iters", "reputation_hist_history", "reputation_bin_edges"}
            assert np.array_equal(hist[k]["reputation_history_iters"], np.arange(1, eng.last_iteration(k) + 1, 5))
            assert np.array_equal(hist[k]["reputation_hist_history"][0].sum(axis=0),
                                  np.histogram(np.zeros(L * L), bins=20, range=(-10, 10))[0])   # R_1 = 0
            assert np.all(hist[k]["reputation_hist_history"].sum(axis=(1, 2)) == L * L)
    finally:
        eng.close()


def _stepwise_expectation(make, T):
    """([replica][t] -> (S_t 0/1, R_t stored values) (L, L)), last: an engine stepped one iteration at a
    time with host copies of both planes (the method of tests/test_gpu_clusters.py)."""
    eng = make()
    try:
        seen = []
        for t in range(1, T + 1):
            seen.append((eng.S[(t - 1) & 1].cpu().numpy() & 1, eng.Rep[(t - 1) & 1].cpu().numpy().copy()))
            eng.step(1)
            eng.all_stopped()
        last = [eng.last_iteration(k) for k in range(eng.R)]
        L = eng.L
        return [{t: (seen[t - 1][0][k].reshape(L, L), seen[t - 1][1][k].reshape(L, L))
                 for t in range(1, last[k] + 1)} for k in range(eng.R)], last
    finally:
        eng.close()


def _assert_histories(hist, planes, last, every, bins, D, lo=-10, hi=10, unit=1.0, t0=1):
    for k, h in enumerate(hist):
        its = np.arange(t0, last[k] + 1, every)
        assert np.array_equal(h["reputation_history_iters"], its), k
        assert h["reputation_hist_history"].dtype == np.int64 and h["reputation_hist_history"].shape == (len(its), 2, bins)
        assert h["reputation_bin_edges"].dtype == np.float64
        assert np.array_equal(h["reputation_bin_edges"], K.edges_of(lo, hi, bins))
        for j, t in enumerate(its):
            S, R8 = planes[k][t]
            want = K.expected_hist(S, R8.astype(np.float64) * unit, bins, lo, hi)
            assert np.array_equal(h["reputation_hist_history"][j], want), (k, t, every)
        if D is None:
            assert "reputation_sum_history" not in h
            continue
        assert h["reputation_unit"] == unit
        want = [K.expected_pair_sums(planes[k][t][1], D) for t in its]
        assert h["reputation_sum_history"].dtype == np.int64 and h["reputation_sum_history"].shape == (len(its),)
        assert np.array_equal(h["reputation_sum_history"], [w[0] for w in want]), (k, every)
        for key, j in (("reputation_pair_rows_history", 1), ("reputation_pair_cols_history", 2)):
            assert h[key].dtype == np.int64 and h[key].shape == (len(its), D + 1), (k, key)
            assert np.array_equal(h[key], np.array([w[j] for w in want]).reshape(len(its), D + 1)), (k, key, every)


def test_in_run_record():
    L, T = 24, 40

    def make():
        seeds = (11, 12, 13)
        reps = [_params(seed=s) for s in seeds]
        init = [reference_init(L, np.random.RandomState(s), S_in_one=np.zeros((L, L), dtype=int) if k == 1 else None)
                for k, s in enumerate(seeds)]   # replica 1 starts all-C: absorbed at t = 1
        return BatchEngine(L, T, reps, use_second_order=True, state_representation="action", rng="mt19937", init=init)

    def run(every, bins=20, max_d=None, others=0):
        eng = make()
        try:
            eng.run(snapshots=False, reputation_every=every, reputation_bins=bins, reputation_max_d=max_d,
                    clusters_every=others, correlations_every=others)
            out = dict(final=[eng.final_state(k) for k in range(3)], hist=eng.histories(),
                       mt=[eng.mt_state_host(k) for k in range(3)], last=[eng.last_iteration(k) for k in range(3)])
            if every:
                out["rep"] = eng.reputation_histories()
                out["rec_rows"] = eng.records["reputation"].out[0].shape[1]
                out["final_hist"] = [eng.reputation_histogram(k) for k in range(3)]
                out["final_pairs"] = [eng.reputation_pair_sums(k) for k in range(3)]
            if others:
                out["clusters"], out["corr"] = eng.cluster_histories(), eng.correlation_histories()
            return out
        finally:
            eng.close()

    planes, last = _stepwise_expectation(make, T)
    assert last[1] == 1 and last[0] > 7
    plain = run(0)
    assert plain["last"] == last
    both = run(0, others=7)
    for every, bins, max_d, others in ((1, 20, L // 2, 0), (7, 256, None, 0), (7, 20, 5, 7)):
        got = run(every, bins, max_d, others)
        _assert_histories(got["rep"], planes, last, every, bins, max_d)
        assert got["rec_rows"] == (T - 1) // every + 1   # one row per recorded iteration
        for k in range(3):   # the final values are those of the state final_state returns
            Q, R, S = got["final"][k]
            assert np.array_equal(got["final_hist"][k], K.expected_hist(S, R, 20, -10, 10)), k
            ws, wr, wc = K.expected_pair_sums(R.astype(np.int64), L // 2)   # unit 1
            s, rows, cols = got["final_pairs"][k]
            assert s == ws and np.array_equal(rows, wr) and np.array_equal(cols, wc), k
        if others:   # the other two records, taken beside this one, are what they are without it
            for a, b in zip(got["clusters"] + got["corr"], both["clusters"] + both["corr"]):
                assert set(a) == set(b) and all(np.array_equal(a[key], b[key]) for key in a)
        # the record does not disturb the run
        for k in range(3):
            for a, b in zip(got["final"][k], plain["final"][k]):
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


def test_record_from_a_later_iteration_and_continued():
    """A run that starts at t0 = 6 records t0, t0 + k, ...; run() again with the same settings keeps
    the record (and, the run being over, adds nothing to it)."""
    L, T, every = 16, 30, 4

    def make():
        return BatchEngine(L, T, [_params(seed=s) for s in (5, 6)], use_second_order=False, rng="mt19937")

    planes, last = _stepwise_expectation(make, T)
    eng = make()
    try:
        kw = dict(snapshots=False, reputation_every=every, reputation_max_d=3)
        eng.step(5)
        eng.run(**kw)
        record = eng.records["reputation"]
        rec, pairs = record.out
        assert rec.shape[1] == (T - 6) // every + 1
        first = eng.reputation_histories()
        eng.run(**kw)
        assert eng.records["reputation"] is record and record.out[0] is rec and record.out[1] is pairs
        hist = eng.reputation_histories()
    finally:
        eng.close()
    _assert_histories(hist, planes, last, every, 20, 3, t0=6)
    for a, b in zip(first, hist):
        assert all(np.array_equal(a[key], b[key]) for key in a)


def test_replica_groups():
    L, T, every, D = 200, 10, 3, 6
    R = next(r for r in range(1, 64) if plan_groups(r, L, 1, 1 << 40)[1] >= 2)   # the planner's first split

    def make():
        return BatchEngine(L, T, [_params(seed=100 + k) for k in range(R)], use_second_order=False, rng="philox")

    eng = make()
    try:
        assert eng.G >= 2, (R, eng.G)
        eng.run(snapshots=False, reputation_every=every, reputation_max_d=D)
        hist = eng.reputation_histories()
        ends = sorted({g["r0"] for g in eng.groups} | {g["r1"] - 1 for g in eng.groups})
        finals = {k: (eng.final_state(k), eng.reputation_histogram(k), eng.reputation_pair_sums(k)) for k in ends}
    finally:
        eng.close()
    planes, last = _stepwise_expectation(make, T)
    _assert_histories(hist, planes, last, every, 20, D)
    for k, ((Q, Rk, S), h, (s, rows, cols)) in finals.items():   # the first and last replica of every group
        assert np.array_equal(h, K.expected_hist(S, Rk, 20, -10, 10)), k
        ws, wr, wc = K.expected_pair_sums(Rk.astype(np.int64), L // 2)
        assert s == ws and np.array_equal(rows, wr) and np.array_equal(cols, wc), k


@pytest.mark.parametrize("name", ["m1_rep_L10_snap", "defaults_L12"])
def test_against_the_references_own_histograms(name, tmp_path, monkeypatch):
    """The reference's fixtures through the drop-in with the record at every iteration: the row of
    iteration i, summed over strategy, is the fixture's rep_hist_i; split by strategy it is
    np.histogram of R_snapshot_i masked by Sn_snapshot_i; the final histogram is rep_hist_final."""
    c = Case(name)
    seen = {}
    close = BatchEngine.close

    def closing(self):   # the drop-in's engine, after its run: the final histogram on the device
        if "final" not in seen and getattr(self, "groups", None) and self.groups[0].get("ctx"):
            seen["final"] = self.reputation_histogram(0)
        close(self)

    monkeypatch.setattr(BatchEngine, "close", closing)
    m = _pinned_model(c)
    m.save_png = False
    m.reputation_history_every = 1
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    lo, hi = c.kwargs.get("R_min", -10), c.kwargs.get("R_max", 10)
    its = ds["reputation_history_iters"]
    assert np.array_equal(its, np.arange(1, len(ds["coop_rate_history"]) + 1))
    assert np.array_equal(ds["reputation_bin_edges"], c.datasets["rep_bins_1"])
    snaps = sorted(int(k[9:]) for k in c.datasets if k.startswith("rep_hist_") and k != "rep_hist_final")
    assert snaps and snaps[0] == 1
    for i in snaps:
        row = ds["reputation_hist_history"][i - 1]
        assert np.array_equal(row.sum(axis=0), c.datasets[f"rep_hist_{i}"]), i
        assert np.array_equal(row, K.expected_hist(c.datasets[f"Sn_snapshot_{i}"], c.datasets[f"R_snapshot_{i}"],
                                                   20, lo, hi)), i
    assert np.array_equal(ds["rep_hist_final"], c.datasets["rep_hist_final"])
    assert np.array_equal(seen["final"].sum(axis=0), c.datasets["rep_hist_final"])
    assert np.array_equal(seen["final"], K.expected_hist(c.Sn, c.R, 20, lo, hi))
    extra = {"reputation_history_iters", "reputation_hist_history", "reputation_bin_edges"}
    assert set(ds) - set(c.datasets) == extra and set(c.datasets) <= set(ds)

    # the option off: the reference's dataset set
    m2 = _pinned_model(c)
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    assert set(read_datasets(fn2)) == set(c.datasets)


def test_dropin_datasets_and_sweep_override(tmp_path, monkeypatch):
    m = spgg_amd.SPGG(L=16, iterations=30, r=3.0)
    m.save_png = False
    m.reputation_history_every = 3
    m.reputation_history_bins = 12
    m.reputation_max_distance = 4
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    its = np.arange(1, len(ds["coop_rate_history"]) + 1, 3)

    def check(ds, its, bins, D, unit):
        assert np.array_equal(ds["reputation_history_iters"], its) and ds["reputation_history_iters"].dtype == np.int64
        assert ds["reputation_hist_history"].shape == (len(its), 2, bins) and ds["reputation_hist_history"].dtype == np.int64
        assert ds["reputation_bin_edges"].dtype == np.float64
        assert np.array_equal(ds["reputation_bin_edges"], K.edges_of(-10, 10, bins))
        assert ds["reputation_sum_history"].shape == (len(its),) and ds["reputation_sum_history"].dtype == np.int64
        for key in ("reputation_pair_rows_history", "reputation_pair_cols_history"):
            assert ds[key].shape == (len(its), D + 1) and ds[key].dtype == np.int64, key
        assert ds["reputation_unit"].dtype == np.float64 and ds["reputation_unit"].size == 1
        assert float(np.ravel(ds["reputation_unit"])[0]) == unit
        # the rows of the reference's snapshot iterations: 1 (the initial population) and 10
        assert its[0] == 1 and its[3] == 10
        for row, i in ((0, 1), (3, 10)):
            Si, Ri = ds[f"Sn_snapshot_{i}"], ds[f"R_snapshot_{i}"]
            assert np.array_equal(ds["reputation_hist_history"][row], K.expected_hist(Si, Ri, bins, -10, 10)), i
            Ki = Ri / unit   # the stored bytes: exact, R is a multiple of the dyadic unit
            assert np.array_equal(Ki, np.round(Ki)) and (i == 1 or Ki.any())
            ws, wr, wc = K.expected_pair_sums(Ki.astype(np.int64), D)
            assert ds["reputation_sum_history"][row] == ws, i
            assert np.array_equal(ds["reputation_pair_rows_history"][row], wr), i
            assert np.array_equal(ds["reputation_pair_cols_history"][row], wc), i

    check(ds, its, 12, 4, 0.5)   # the drop-in's default rep_gain_C = 0.5: unit 1/2
    m2 = spgg_amd.SPGG(L=16, iterations=30, r=3.0)   # the default 0: today's dataset names
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    plain = read_datasets(fn2)
    extra = set(spgg_amd.spgg.REPUTATION_DATASETS)
    assert not extra & set(plain)
    assert set(ds) - set(plain) == extra and set(plain) <= set(ds)

    # the sweep's batched runner takes the same three among its model overrides
    from spgg_amd import sweep as SW
    monkeypatch.chdir(tmp_path)
    params = [(3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning"),
              (4.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning")]
    SW.run_batch(params, seeds=[1, 2], save_png=False, verbose=False, L=16, iterations=12,
                 reputation_history_every=3, reputation_history_bins=7, reputation_max_distance=2)
    for p in params:
        got = read_datasets(str(tmp_path / SW.get_folder_name(*p) / "data" / "experiment_data.h5"))
        check(got, np.arange(1, len(got["coop_rate_history"]) + 1, 3), 7, 2, 1.0)   # the tuples' gain 1.0: unit 1
