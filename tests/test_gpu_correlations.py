"""Device pair counts (spgg_correlations, ABI v18) against the host: final counts
(BatchEngine.pair_counts), the in-run record (run(correlations_every=k) / correlation_histories),
the drop-in's datasets and the fallback above the supported side.  Expectations are np.roll on
host copies of S (tests/_correlations.py); every count comparison is exact (integers).  "The
record does not disturb the run" is held as tests/test_gpu_clusters.py holds it: bit identity for
the final state, the MT19937 key and every history outside that file's ORDER_DEPENDENT set, and
that file's SUM_ORDER_TOL (derived there: two summation orders of n = L*L f64 terms) for the
histories the step kernels sum with atomics, which differ between two identical runs already."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib  # noqa: E402
from spgg_amd.engine import BatchEngine, host_pair_counts, plan_groups, reference_init  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402

from tests import _clusters as CL  # noqa: E402
from tests import _correlations as K  # noqa: E402
from tests.test_gpu_clusters import (ORDER_DEPENDENT, SUM_ORDER_TOL, _params, _pattern_engine,  # noqa: E402
                                     _stepwise_expectation)


def _check_engine(eng, planes, names, distances=(None, 0, 1)):
    L = eng.L
    for k, S in enumerate(planes):
        mask = (S & 1) == 0
        want = K.expected_pair_counts(mask, L // 2)
        for max_d in distances:
            if max_d is not None and max_d > L // 2:
                continue
            D = L // 2 if max_d is None else max_d
            got = eng.pair_counts(k, max_d)
            assert got.dtype == np.int64 and got.shape == (2, D + 1), (names[k], max_d, got.shape)
            assert np.array_equal(got, want[:, :D + 1]), (names[k], max_d)
            assert got[0, 0] == got[1, 0] == int(mask.sum()), (names[k], max_d)
        assert np.array_equal(eng.final_state(k)[2], S & 1)


@pytest.mark.parametrize("L", [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 96, 127, 129])
def test_patterns(L):
    names, planes = K.planes_of(L)   # one batch: odd L puts the replica planes at odd byte offsets
    eng = _pattern_engine(L, planes)
    try:
        _check_engine(eng, planes, names)
    finally:
        eng.close()


def test_side_200():
    L = 200
    masks = [("serpentine", CL.serpentines(L)[1]), ("spiral", CL.spiral(L)), ("random0.593", CL.random_mask(L, 0.593, 3))]
    planes = [np.where(m, 0, 1).astype(np.uint8) for _, m in masks]
    eng = _pattern_engine(L, planes)
    try:
        _check_engine(eng, planes, [n for n, _ in masks])
    finally:
        eng.close()


def _random_plane(L, seed):
    rs = np.random.RandomState(seed)
    return (np.where(rs.rand(L, L) < 0.5, 0, 1) | (rs.randint(0, 16, (L, L)) << 1)).astype(np.uint8)


# 256 / 257: the last side of the kernel instance with the small LDS declaration and the first of
# the one that may take a whole CU's; 1000: cfg5; None: correlations_max_side
@pytest.mark.parametrize("L", [256, 257, 1000, None])
def test_sizes(L):
    probe = _pattern_engine(2, [np.zeros((2, 2), dtype=np.uint8)])
    try:
        side = probe.correlations_max_side
    finally:
        probe.close()
    assert side >= 1000
    L = side if L is None else L
    planes = [_random_plane(L, L)]
    eng = _pattern_engine(L, planes)
    try:
        assert eng.correlations_max_side == side
        _check_engine(eng, planes, [f"random{L}"], distances=(None,))
    finally:
        eng.close()


def test_above_the_supported_side():
    probe = _pattern_engine(2, [np.zeros((2, 2), dtype=np.uint8)])
    try:
        side = probe.correlations_max_side
    finally:
        probe.close()
    L = side + 1
    S = _random_plane(L, 5)
    eng = _pattern_engine(L, [S])
    try:
        out = torch.zeros(4, dtype=torch.int32, device=eng.dev)
        rc = eng.lib.spgg_correlations(eng.ctx, 1, 1, out.data_ptr(), 4, eng.stream)
        assert rc == _lib.E_ARG
        assert str(side) in eng.lib.spgg_last_error(eng.ctx).decode()
        assert not out.cpu().numpy().any()
        want = K.expected_pair_counts((S & 1) == 0, 5)
        for max_d in (5, 0):
            got = eng.pair_counts(0, max_d)
            assert np.array_equal(got, want[:, :max_d + 1]), max_d
            assert np.array_equal(got, host_pair_counts(S, max_d))
        with pytest.raises(ValueError, match=str(side)):
            eng.run(snapshots=False, correlations_every=1)
        assert eng.t == 1   # nothing was enqueued
    finally:
        eng.close()


def test_argument_errors():
    L = 10
    eng = _pattern_engine(L, [_random_plane(L, 1)])
    try:
        out = torch.zeros(2 * (L // 2 + 2), dtype=torch.int32, device=eng.dev)
        call = eng.lib.spgg_correlations
        assert call(eng.ctx, 0, 1, out.data_ptr(), out.numel(), eng.stream) == _lib.E_ARG          # t < 1
        assert call(eng.ctx, 1, -1, out.data_ptr(), out.numel(), eng.stream) == _lib.E_ARG         # max_d < 0
        assert call(eng.ctx, 1, L // 2 + 1, out.data_ptr(), out.numel(), eng.stream) == _lib.E_ARG  # max_d > L / 2
        assert call(eng.ctx, 1, 1, None, out.numel(), eng.stream) == _lib.E_ARG                    # null out
        side = ctypes.c_int32()
        assert eng.lib.spgg_correlations_max_side(eng.ctx, None) == _lib.E_ARG
        assert eng.lib.spgg_correlations_max_side(eng.ctx, ctypes.byref(side)) == _lib.OK
        assert side.value == eng.correlations_max_side
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()
        for bad in (dict(correlations_every=-1), dict(correlations_every=1, correlations_max_d=L // 2 + 1),
                    dict(correlations_every=1, correlations_max_d=-1)):
            with pytest.raises(ValueError):
                eng.run(snapshots=False, **bad)
            assert eng.t == 1
        with pytest.raises(ValueError):
            eng.pair_counts(0, L // 2 + 1)
        with pytest.raises(ValueError):
            eng.correlation_histories()
    finally:
        eng.close()


def _assert_histories(hist, planes, last, every, D, t0=1):
    for k, h in enumerate(hist):
        its = np.arange(t0, last[k] + 1, every)
        assert np.array_equal(h["correlation_history_iters"], its), k
        want = np.array([K.expected_pair_counts(planes[k][t] == 0, D) for t in its], dtype=np.int64).reshape(-1, 2, D + 1)
        for j, key in enumerate(("pair_count_rows_history", "pair_count_cols_history")):
            assert h[key].dtype == np.int64 and h[key].shape == (len(its), D + 1), (k, key, h[key].shape)
            assert np.array_equal(h[key], want[:, j]), (k, key, every)


def test_in_run_record():
    L, T = 24, 40

    def make():
        seeds = (11, 12, 13)
        reps = [_params(seed=s) for s in seeds]
        init = [reference_init(L, np.random.RandomState(s), S_in_one=np.zeros((L, L), dtype=int) if k == 1 else None)
                for k, s in enumerate(seeds)]   # replica 1 starts all-C: absorbed at t = 1
        return BatchEngine(L, T, reps, use_second_order=True, state_representation="action", rng="mt19937", init=init)

    def run(every, max_d=None, clusters_every=0):
        eng = make()
        try:
            eng.run(snapshots=False, correlations_every=every, correlations_max_d=max_d, clusters_every=clusters_every)
            out = dict(final=[eng.final_state(k) for k in range(3)], hist=eng.histories(),
                       mt=[eng.mt_state_host(k) for k in range(3)], last=[eng.last_iteration(k) for k in range(3)])
            if every:
                out["corr"] = eng.correlation_histories()
                out["rec_rows"] = eng.records["correlations"].out[0].shape[1]
                out["final_counts"] = [eng.pair_counts(k) for k in range(3)]
            if clusters_every:
                out["clusters"] = eng.cluster_histories()
            return out
        finally:
            eng.close()

    planes, last = _stepwise_expectation(make, T)
    assert last[1] == 1 and last[0] > 7
    plain = run(0)
    assert plain["last"] == last
    for every, max_d, clusters_every in ((1, None, 0), (7, 5, 0), (7, None, 7)):
        got = run(every, max_d, clusters_every)
        D = L // 2 if max_d is None else max_d
        _assert_histories(got["corr"], planes, last, every, D)
        assert got["rec_rows"] == (T - 1) // every + 1   # one row per recorded iteration, not T + 2
        for k in range(3):   # the final counts are those of the state final_state returns
            assert np.array_equal(got["final_counts"][k], K.expected_pair_counts(got["final"][k][2] == 0, L // 2))
        if clusters_every:
            for k, h in enumerate(got["clusters"]):
                its = np.arange(1, last[k] + 1, clusters_every)
                assert np.array_equal(h["cluster_history_iters"], its)
                want = [CL.expected_record(planes[k][t], False) for t in its]
                assert [(a, b, c) for a, b, c in zip(h["cluster_count_history"], h["largest_cluster_history"],
                                                     h["cd_bond_history"])] == want, k
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


def test_replica_groups():
    L, T, every = 200, 10, 3
    R = next(r for r in range(1, 64) if plan_groups(r, L, 1, 1 << 40)[1] >= 2)   # the planner's first split

    def make():
        return BatchEngine(L, T, [_params(seed=100 + k) for k in range(R)], use_second_order=False, rng="philox")

    eng = make()
    try:
        assert eng.G >= 2, (R, eng.G)
        eng.run(snapshots=False, correlations_every=every)
        hist = eng.correlation_histories()
        counts = [eng.pair_counts(k) for k in range(R)]
        finals = [eng.final_state(k)[2] for k in range(R)]
    finally:
        eng.close()
    planes, last = _stepwise_expectation(make, T)
    _assert_histories(hist, planes, last, every, L // 2)
    for k in range(R):   # replicas of every group, through each group's own launch
        assert np.array_equal(counts[k], K.expected_pair_counts(finals[k] == 0, L // 2)), k


def test_dropin_datasets(tmp_path):
    m = spgg_amd.SPGG(L=16, iterations=30, r=3.0)
    m.save_png = False
    m.correlation_history_every = 5
    m.correlation_max_distance = 4
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    n_it = len(ds["coop_rate_history"])
    its = np.arange(1, n_it + 1, 5)
    assert np.array_equal(ds["correlation_history_iters"], its) and ds["correlation_history_iters"].dtype == np.int64
    for key in ("pair_count_rows_history", "pair_count_cols_history"):
        assert ds[key].shape == (len(its), 5) and ds[key].dtype == np.int64, key
    want = K.expected_pair_counts(ds["Sn_snapshot_1"] == 0, 4)   # the record's first row: the initial population
    assert np.array_equal(ds["pair_count_rows_history"][0], want[0])
    assert np.array_equal(ds["pair_count_cols_history"][0], want[1])

    m2 = spgg_amd.SPGG(L=16, iterations=30, r=3.0)   # the default 0: today's dataset names
    m2.save_png = False
    m2.folder = str(tmp_path / "plain")
    fn2 = str(tmp_path / "plain.h5")
    m2.run(fn2)
    plain = read_datasets(fn2)
    extra = {"correlation_history_iters", "pair_count_rows_history", "pair_count_cols_history"}
    assert not extra & set(plain)
    assert set(ds) - set(plain) == extra and set(plain) <= set(ds)
