"""Device cluster labelling (spgg_clusters, ABI v17) against the host: final cluster sizes
(BatchEngine.cluster_sizes), the in-run record (run(clusters_every=k) / cluster_histories), the
drop-in's datasets and the fallback above the supported side.  Expectations are scipy's
labelling of host copies of S (tests/_clusters.py; periodic: merged across the seam there);
every cluster comparison is exact (integers).  The one departure from "bit-identical to a run
without the record": the histories the step kernels sum with f64 atomics differ between two
identical runs already (see ORDER_DEPENDENT), so they are held to the summation-order bound
and everything else -- final state, MT19937 key, every other history -- to bit identity."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib  # noqa: E402
from spgg_amd.engine import BatchEngine, InitState, ReplicaParams, plan_groups, reference_init  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402

from tests import _clusters as K  # noqa: E402

SIDE = 200


def _params(**kw):
    base = dict(c=1, cost=1, alpha=0.8, gamma=0.9, epsilon=0.5, epsilon_decay=0.99, epsilon_min=0.01,
                lambda_epsilon=0.01, delta_R_D=1, R_min=-10, R_max=10, rep_gain_C=1.0,
                reward_weight_payoff=0.95, influence_factor=1.0, r=3.0)
    base.update(kw)
    return ReplicaParams(**base)


def _pattern_engine(L, planes):
    """An engine whose replicas start from the given uint8 S planes; nothing is stepped."""
    init = [InitState(Q=np.zeros((L, L, 2, 2)), S=S) for S in planes]
    return BatchEngine(L, 4, [_params(seed=k) for k in range(len(planes))], use_second_order=False,
                       rng="philox", init=init)


def _check_engine(eng, planes, names):
    for periodic in (False, True):
        for k, S in enumerate(planes):
            want = K.expected_sizes((S & 1) == 0, periodic)
            got = eng.cluster_sizes(k, periodic=periodic)
            assert got.dtype == np.int64 and got.shape == want.shape, (names[k], periodic, got.shape, want.shape)
            assert np.array_equal(got, want), (names[k], periodic)
            assert np.array_equal(eng.final_state(k)[2], S & 1)
        rec = eng._final_cache["cluster_record", periodic]   # the record of the same launch
        for k, S in enumerate(planes):
            assert tuple(rec[k]) == K.expected_record(S, periodic), (names[k], periodic, rec[k])


@pytest.mark.parametrize("L", [1, 2, 3, 5, 13, 16, 33, 64])
def test_patterns(L):
    masks = K.pattern_masks(L, seed=L)
    names = [n for n, _ in masks] + ["dirty_bits"]
    planes = [np.where(m, 0, 1).astype(np.uint8) for _, m in masks]
    rs = np.random.RandomState(7 + L)   # bits 1-4 are bookkeeping of the step: only bit 0 counts
    planes.append((np.where(K.random_mask(L, 0.6, 99 + L), 0, 1) | (rs.randint(0, 16, (L, L)) << 1)).astype(np.uint8))
    eng = _pattern_engine(L, planes)
    try:
        _check_engine(eng, planes, names)
    finally:
        eng.close()


def test_patterns_supported_side():
    L = SIDE
    masks = [("serpentine", K.serpentines(L)[1]), ("spiral", K.spiral(L)),
             ("random0.593", K.random_mask(L, 0.593, 3)), ("all_c", np.ones((L, L), dtype=bool))]
    planes = [np.where(m, 0, 1).astype(np.uint8) for _, m in masks]
    eng = _pattern_engine(L, planes)
    try:
        assert eng.clusters_max_side == SIDE
        _check_engine(eng, planes, [n for n, _ in masks])
    finally:
        eng.close()


def _stepwise_expectation(make, T):
    """[replica][t] -> S_t (0/1, (L, L)) of an engine stepped one iteration at a time, for
    t = 1 .. last_iteration of the replica."""
    eng = make()
    try:
        seen = []
        for t in range(1, T + 1):
            seen.append(eng.S[(t - 1) & 1].cpu().numpy() & 1)
            eng.step(1)
            eng.all_stopped()
        last = [eng.last_iteration(k) for k in range(eng.R)]
        return [{t: seen[t - 1][k].reshape(eng.L, eng.L) for t in range(1, last[k] + 1)} for k in range(eng.R)], last
    finally:
        eng.close()


def _assert_histories(hist, planes, last, every, periodic):
    for k, h in enumerate(hist):
        its = np.arange(1, last[k] + 1, every)
        assert np.array_equal(h["cluster_history_iters"], its), k
        want = np.array([K.expected_record(planes[k][t], periodic) for t in its], dtype=np.int64).reshape(-1, 3)
        for j, key in enumerate(("cluster_count_history", "largest_cluster_history", "cd_bond_history")):
            assert h[key].dtype == np.int64
            assert np.array_equal(h[key], want[:, j]), (k, key, every, periodic)


# Histories that are means of f64 terms the step kernels add with atomics in arrival order, over
# the 3 x 8-row tiles of an L = 24 replica: two IDENTICAL runs of the engine (clusters_every = 0
# both times, the parent commit's code path) differ in them by 1.5e-16 .. 4.6e-16 relative
# (measured on MI355X: 27 of the datasets of the two running replicas), so "bit-identical to a
# run without the record" can hold only for everything else -- the final state, the MT19937 key
# and every other history, which are compared bit for bit.  For these, two summation orders of
# n = L*L terms differ by at most 2 (n - 1) u sum|x| (u = 2^-53): relative to the mean, 2 n u
# times sum|x| / |sum x|, with an absolute floor of 2 n u for sums that cancel (|x| <= 1 here:
# normalised rewards / Q-values of order 1; reputation ratios are all positive).
ORDER_DEPENDENT = {"reputation_reward_ratio", "avg_reward_C_history", "avg_reward_D_history",
                   "neighbor_influence_percent"} | {
    f"{g}_q_{s}_{a}_history" for g in ("cooperators", "defectors", "avg") for s in ("s0", "s1") for a in ("c", "d")}
SUM_ORDER_TOL = dict(rtol=2 * 24 * 24 * 2.0 ** -53, atol=2 * 24 * 24 * 2.0 ** -53)


def test_in_run_record():
    L, T = 24, 40

    def make():
        seeds = (11, 12, 13)
        reps = [_params(seed=s) for s in seeds]
        init = [reference_init(L, np.random.RandomState(s), S_in_one=np.zeros((L, L), dtype=int) if k == 1 else None)
                for k, s in enumerate(seeds)]   # replica 1 starts all-C: absorbed at t = 1
        return BatchEngine(L, T, reps, use_second_order=True, state_representation="action", rng="mt19937", init=init)

    def run(every, periodic):
        eng = make()
        try:
            eng.run(snapshots=False, clusters_every=every, clusters_periodic=periodic)
            out = dict(final=[eng.final_state(k) for k in range(3)], hist=eng.histories(),
                       mt=[eng.mt_state_host(k) for k in range(3)], last=[eng.last_iteration(k) for k in range(3)])
            if every:
                out["clusters"] = eng.cluster_histories()
                out["rec_rows"] = eng.records["clusters"].out[0].shape[1]
            return out
        finally:
            eng.close()

    planes, last = _stepwise_expectation(make, T)
    assert last[1] == 1 and last[0] > 7
    plain = run(0, False)
    assert plain["last"] == last
    for periodic in (False, True):
        for every in (1, 7):
            got = run(every, periodic)
            _assert_histories(got["clusters"], planes, last, every, periodic)
            assert got["rec_rows"] == (T - 1) // every + 1   # one row per recorded iteration, not T + 2
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
    L, T, every = SIDE, 10, 3
    R = next(r for r in range(1, 64) if plan_groups(r, L, 1, 1 << 40)[1] >= 2)   # the planner's first split

    def make():
        return BatchEngine(L, T, [_params(seed=100 + k) for k in range(R)], use_second_order=False, rng="philox")

    eng = make()
    try:
        assert eng.G >= 2, (R, eng.G)
        eng.run(snapshots=False, clusters_every=every)
        hist = eng.cluster_histories()
        sizes = [eng.cluster_sizes(k) for k in range(R)]
        finals = [eng.final_state(k)[2] for k in range(R)]
    finally:
        eng.close()
    planes, last = _stepwise_expectation(make, T)
    _assert_histories(hist, planes, last, every, False)
    for k in range(R):   # replicas of every group, through each group's own launch
        assert np.array_equal(sizes[k], K.expected_sizes(finals[k] == 0)), k


def test_dropin_datasets(tmp_path):
    m = spgg_amd.SPGG(L=16, iterations=30, r=3.0)
    m.save_png = False
    m.cluster_history_every = 5
    m.folder = str(tmp_path)
    fn = str(tmp_path / "experiment_data.h5")
    m.run(fn)
    ds = read_datasets(fn)
    n_it = len(ds["coop_rate_history"])
    its = np.arange(1, n_it + 1, 5)
    assert np.array_equal(ds["cluster_history_iters"], its)
    for key in ("cluster_count_history", "largest_cluster_history", "cd_bond_history"):
        assert ds[key].shape == its.shape and ds[key].dtype == np.int64, key
    assert np.array_equal(ds["cluster_sizes"], K.expected_sizes(ds["Sn_final"] == 0))
    assert np.array_equal(ds["cluster_sizes"], spgg_amd.cluster_sizes(ds["Sn_final"]))
    # the record's first row is the initial population's
    assert (ds["cluster_count_history"][0] >= 1) == bool(np.any(ds["Sn_snapshot_1"] == 0))
    assert (ds["cluster_count_history"][0], ds["largest_cluster_history"][0], ds["cd_bond_history"][0]) == \
        K.expected_record(ds["Sn_snapshot_1"])


def test_above_the_supported_side():
    L = SIDE + 1
    eng = BatchEngine(L, 4, [_params(seed=5)], use_second_order=False, rng="philox")
    try:
        assert eng.clusters_max_side == SIDE
        rec = torch.zeros(3, dtype=torch.int32, device=eng.dev)
        rc = eng.lib.spgg_clusters(eng.ctx, 1, 0, None, rec.data_ptr(), 3, eng.stream)
        assert rc == _lib.E_ARG
        assert str(SIDE) in eng.lib.spgg_last_error(eng.ctx).decode()
        S = eng.final_state(0)[2]
        for periodic in (False, True):
            assert np.array_equal(eng.cluster_sizes(0, periodic=periodic), K.expected_sizes(S == 0, periodic))
        with pytest.raises(ValueError, match=str(SIDE)):
            eng.run(snapshots=False, clusters_every=1)
        assert eng.t == 1   # nothing was enqueued
    finally:
        eng.close()
