"""Tiled device cluster labelling (spgg_clusters_tiled, within ABI v19) against the host and against
the one-workgroup kernel: written S planes through the raw ABI call at many tile sides, the
library's tile at sides 201 / 264 / 1000, bit-equality with spgg_clusters on stepped engines, the
in-run record (run(clusters_every=k, clusters_tiled=...)), lattices above side 200, replica groups,
cfg5's shape, the drop-in and the sweep.  Expectations are scipy's labelling of host copies of S
(tests/_clusters.py); every cluster comparison is exact (integers).  The histories the step kernels
sum with f64 atomics are held to the summation-order bound of tests/test_gpu_clusters.py, everything
else of a recorded run to bit identity with a run without the record."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")
pytestmark = pytest.mark.gpu

import spgg_amd  # noqa: E402
from spgg_amd import _lib  # noqa: E402
from spgg_amd.engine import BatchEngine, plan_groups, reference_init  # noqa: E402
from spgg_amd.h5io import read_datasets  # noqa: E402
from spgg_amd.spgg import CLUSTER_DATASETS  # noqa: E402

from tests import _clusters as K  # noqa: E402
from tests import test_gpu_clusters as G  # noqa: E402  (its engines, stepwise expectation and bounds)

GARBAGE = 0x7f7f7f7f   # the workspace's contents are undefined before a call


def _workspace(eng):
    words = ctypes.c_int64(0)
    assert eng.lib.spgg_clusters_tiled_workspace(eng.ctx, ctypes.byref(words)) == _lib.OK
    assert words.value == 2 * eng.n + 8
    return torch.full((eng.R, words.value), GARBAGE, dtype=torch.int32, device=eng.dev)


def _call(eng, fn, *args):
    """(sizes (R, n), rec (R, 3)) int64 of one labelling call per replica group (the planner splits
    wide lattices), each on its context's replicas; a tensor among args is passed as the group's slice."""
    sizes = torch.full((eng.R, eng.n), GARBAGE, dtype=torch.int32, device=eng.dev)
    rec = torch.full((eng.R, 3), GARBAGE, dtype=torch.int32, device=eng.dev)
    torch.cuda.synchronize(eng.dev)
    stream = torch.cuda.current_stream(eng.dev).cuda_stream
    for g in eng.groups:
        r0 = g["r0"]
        a = [x[r0].data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
        rc = fn(g["ctx"], eng.t, *a, sizes[r0].data_ptr(), rec[r0].data_ptr(), 3, stream)
        assert rc == _lib.OK, eng.lib.spgg_last_error(g["ctx"])
    torch.cuda.synchronize(eng.dev)
    return sizes.cpu().numpy().astype(np.int64), rec.cpu().numpy().astype(np.int64)


def _tiled(eng, periodic, tile, work=None):
    work = _workspace(eng) if work is None else work
    return _call(eng, eng.lib.spgg_clusters_tiled, int(periodic), tile, work)


def _assert_planes(eng, planes, names, periodic, tile, work=None):
    sizes, rec = _tiled(eng, periodic, tile, work)
    for k, S in enumerate(planes):
        mask = (S & 1) == 0
        want = K.expected_sizes(mask, periodic)
        tag = (names[k], eng.L, tile, periodic)
        assert tuple(rec[k]) == K.expected_record(S, periodic), (tag, rec[k])
        assert np.array_equal(sizes[k][sizes[k] > 0], want), tag
        assert not np.any(sizes[k][~mask.ravel()]), tag   # representatives are cooperators


@pytest.mark.parametrize("L", [1, 2, 3, 5, 13, 16, 33, 64])
def test_patterns(L):
    masks = K.pattern_masks(L, seed=L)
    names = [n for n, _ in masks] + ["dirty_bits"]
    planes = [np.where(m, 0, 1).astype(np.uint8) for _, m in masks]
    rs = np.random.RandomState(7 + L)   # bits 1-4 are bookkeeping of the step: only bit 0 counts
    planes.append((np.where(K.random_mask(L, 0.6, 99 + L), 0, 1) | (rs.randint(0, 16, (L, L)) << 1)).astype(np.uint8))
    eng = G._pattern_engine(L, planes)
    try:
        work = _workspace(eng)
        for tile in (8, 16):
            for periodic in (False, True):
                _assert_planes(eng, planes, names, periodic, tile, work)   # the workspace is reused as it was left
        rec = torch.zeros((eng.R, 3), dtype=torch.int32, device=eng.dev)
        torch.cuda.synchronize(eng.dev)
        for tile in (7, 201, -1):
            rc = eng.lib.spgg_clusters_tiled(eng.ctx, 1, 0, tile, work.data_ptr(), None, rec.data_ptr(), 3, eng.stream)
            assert rc == _lib.E_ARG and "8 .. 200" in eng.lib.spgg_last_error(eng.ctx).decode(), tile
        assert eng.lib.spgg_clusters_tiled(eng.ctx, 1, 0, 8, None, None, rec.data_ptr(), 3, eng.stream) == _lib.E_ARG
        assert eng.lib.spgg_clusters_tiled(eng.ctx, 1, 0, 8, work.data_ptr(), None, None, 3, eng.stream) == _lib.E_ARG
        torch.cuda.synchronize(eng.dev)
        assert not rec.cpu().numpy().any()   # a refused call enqueues nothing
    finally:
        eng.close()


@pytest.mark.parametrize("L", [201, 264, 1000])
def test_library_tile(L):
    masks = [("serpentine", K.serpentines(L)[1]), ("spiral", K.spiral(L)), ("random0.593", K.random_mask(L, 0.593, 3)),
             ("all_c", np.ones((L, L), dtype=bool)), ("all_d", np.zeros((L, L), dtype=bool))]
    planes = [np.where(m, 0, 1).astype(np.uint8) for _, m in masks]
    eng = G._pattern_engine(L, planes)
    try:
        for periodic in (False, True):
            _assert_planes(eng, planes, [n for n, _ in masks], periodic, 0)
        sizes, rec = _tiled(eng, False, 0)
        assert tuple(rec[3]) == (1, L * L, 0) and sizes[3][0] == L * L and not sizes[3][1:].any()   # one counter
        assert tuple(rec[4]) == (0, 0, 0) and not sizes[4].any()
    finally:
        eng.close()


@pytest.mark.parametrize("L", [24, 200])
def test_agrees_with_the_lds_kernel(L):
    eng = BatchEngine(L, 8, [G._params(seed=40 + k) for k in range(2)], use_second_order=True, rng="philox")
    try:
        eng.step(3)
        for periodic in (False, True):
            sizes, rec = _call(eng, eng.lib.spgg_clusters, int(periodic))
            assert rec[:, 0].min() >= 1
            for tile in (8, 64, 200):
                s2, r2 = _tiled(eng, periodic, tile)
                assert np.array_equal(r2, rec), (L, tile, periodic, r2, rec)
                assert np.array_equal(s2, sizes), (L, tile, periodic)
    finally:
        eng.close()


def test_in_run_record_at_many_tiles():
    L, T = 24, 40

    def make():
        seeds = (11, 12, 13)
        reps = [G._params(seed=s) for s in seeds]
        init = [reference_init(L, np.random.RandomState(s), S_in_one=np.zeros((L, L), dtype=int) if k == 1 else None)
                for k, s in enumerate(seeds)]   # replica 1 starts all-C: absorbed at t = 1
        return BatchEngine(L, T, reps, use_second_order=True, state_representation="action", rng="mt19937", init=init)

    def run(every, periodic, tiled):
        eng = make()
        try:
            eng.run(snapshots=False, clusters_every=every, clusters_periodic=periodic, clusters_tiled=tiled)
            out = dict(final=[eng.final_state(k) for k in range(3)], hist=eng.histories(),
                       mt=[eng.mt_state_host(k) for k in range(3)], last=[eng.last_iteration(k) for k in range(3)])
            if every:
                out["clusters"] = eng.cluster_histories()
                out["key"] = eng.records["clusters"].key
            return out
        finally:
            eng.close()

    planes, last = G._stepwise_expectation(make, T)
    assert last[1] == 1 and last[0] > 7
    plain = run(0, False, False)
    assert plain["last"] == last
    for periodic in (False, True):
        for every in (1, 7):
            got = run(every, periodic, 8)
            lds = run(every, periodic, False)
            assert got["key"] == (every, periodic, 8) and lds["key"] == (every, periodic, None)
            G._assert_histories(got["clusters"], planes, last, every, periodic)
            for a, b in zip(got["clusters"], lds["clusters"]):
                assert set(a) == set(b) == set(CLUSTER_DATASETS)
                for key in a:
                    assert np.array_equal(a[key], b[key]), key
            for k in range(3):   # the record does not disturb the run
                for a, b in zip(got["final"][k], plain["final"][k]):
                    assert np.array_equal(a, b)
                assert np.array_equal(got["mt"][k][0], plain["mt"][k][0]) and got["mt"][k][1] == plain["mt"][k][1]
                assert set(got["hist"][k]) == set(plain["hist"][k])
                for key, v in plain["hist"][k].items():
                    g = got["hist"][k][key]
                    if key in G.ORDER_DEPENDENT:
                        assert g.shape == v.shape, (k, key)
                        np.testing.assert_allclose(g, v, equal_nan=True, err_msg=f"{k} {key}", **G.SUM_ORDER_TOL)
                    else:
                        assert np.array_equal(g, v, equal_nan=True), (k, key)


def test_above_side_200_in_run():
    L, T = G.SIDE + 1, 4

    def make():
        return BatchEngine(L, T, [G._params(seed=5)], use_second_order=False, rng="philox")

    planes, last = G._stepwise_expectation(make, T)
    eng = make()
    try:
        assert eng.clusters_max_side == G.SIDE and getattr(eng, "_clusters_work", None) is None
        eng.run(snapshots=False, clusters_every=1, clusters_tiled=True)
        assert eng._clusters_work is not None and tuple(eng._clusters_work.shape) == (1, 2 * L * L + 8)
        hist = eng.cluster_histories()
        assert len(hist[0]["cluster_history_iters"]) == 4
        G._assert_histories(hist, planes, last, 1, False)
        S = eng.final_state(0)[2]
        for periodic in (False, True):
            assert np.array_equal(eng.cluster_sizes(0, periodic=periodic), K.expected_sizes(S == 0, periodic))
            assert tuple(eng._final_cache["cluster_record", periodic][0]) == K.expected_record(S, periodic)
    finally:
        eng.close()
    eng = make()   # the final sizes alone take the device path too
    try:
        S = eng.final_state(0)[2]
        assert np.array_equal(eng.cluster_sizes(0), K.expected_sizes(S == 0))
        assert eng._clusters_work is not None
    finally:
        eng.close()


def test_replica_groups():
    L, T, every = 208, 6, 3
    R = next(r for r in range(1, 64) if plan_groups(r, L, 1, 1 << 40)[1] >= 2)   # the planner's first split

    def make():
        return BatchEngine(L, T, [G._params(seed=100 + k) for k in range(R)], use_second_order=False, rng="philox")

    eng = make()
    try:
        assert eng.G >= 2, (R, eng.G)
        eng.run(snapshots=False, clusters_every=every, clusters_tiled=True)
        hist = eng.cluster_histories()
        sizes = [eng.cluster_sizes(k) for k in range(R)]
        finals = [eng.final_state(k)[2] for k in range(R)]
    finally:
        eng.close()
    planes, last = G._stepwise_expectation(make, T)
    G._assert_histories(hist, planes, last, every, False)
    for k in range(R):   # replicas of every group, through each group's own launches and workspace slice
        assert np.array_equal(sizes[k], K.expected_sizes(finals[k] == 0)), k


def test_cfg5_shape():
    L, T = 1000, 6

    def make():
        return BatchEngine(L, T, [G._params(seed=9)], use_second_order=False, rng="philox")

    planes, last = G._stepwise_expectation(make, T)
    eng = make()
    try:
        eng.run(snapshots=False, clusters_every=2, clusters_tiled=True)
        hist = eng.cluster_histories()
        assert hist[0]["cluster_history_iters"].tolist() == [1, 3, 5]
        G._assert_histories(hist, planes, last, 2, False)
        S = eng.final_state(0)[2]
        assert np.array_equal(eng.cluster_sizes(0), K.expected_sizes(S == 0))
    finally:
        eng.close()


def test_validation_enqueues_nothing():
    eng = BatchEngine(24, 8, [G._params(seed=3)], use_second_order=False, rng="philox")
    try:
        with pytest.raises(ValueError, match="clusters_every"):
            eng.run(snapshots=False, clusters_tiled=True)
        for tile in (7, 201):
            with pytest.raises(ValueError, match="8 .. 200"):
                eng.run(snapshots=False, clusters_every=2, clusters_tiled=tile)
        assert eng.t == 1 and "clusters" not in eng.records and getattr(eng, "_clusters_work", None) is None
        eng.run(snapshots=False, clusters_every=2, clusters_tiled=8)
        first = eng.records["clusters"]
        assert first.key == (2, False, 8)
    finally:
        eng.close()


def _dropin(tmp_path, name, S, Q, state, **options):
    m = spgg_amd.SPGG(L=16, iterations=30, r=3.0, S_in_one=S.copy())
    m.q_table = Q.copy()
    m.save_png = False
    m.folder = str(tmp_path / name)
    for key, value in options.items():
        setattr(m, key, value)
    np.random.set_state(state)
    fn = str(tmp_path / f"{name}.h5")
    m.run(fn)
    return read_datasets(fn)


def test_dropin_and_sweep(tmp_path, monkeypatch):
    rs = np.random.RandomState(21)
    S, Q = rs.randint(0, 2, size=(16, 16)), rs.uniform(-0.01, 0.01, size=(16, 16, 2, 2))
    state = np.random.RandomState(22).get_state()
    tiled = _dropin(tmp_path, "tiled", S, Q, state, cluster_history_every=5, cluster_history_tiled=8)
    lds = _dropin(tmp_path, "lds", S, Q, state, cluster_history_every=5)
    assert set(tiled) == set(lds) and set(CLUSTER_DATASETS) <= set(tiled)
    its = np.arange(1, len(tiled["coop_rate_history"]) + 1, 5)
    assert np.array_equal(tiled["cluster_history_iters"], its)
    for key in CLUSTER_DATASETS + ("cluster_sizes", "Sn_final", "coop_rate_history"):
        assert np.array_equal(tiled[key], lds[key]), key
    assert (tiled["cluster_count_history"][0], tiled["largest_cluster_history"][0], tiled["cd_bond_history"][0]) == \
        K.expected_record(S)

    from spgg_amd import sweep as SW
    combo = (3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning")
    got = {}
    for name, options in (("a", dict(cluster_history_tiled=8)), ("b", {})):
        (tmp_path / name).mkdir()
        monkeypatch.chdir(tmp_path / name)
        SW.run_batch([combo], seeds=[1], save_png=False, verbose=False, L=16, iterations=20, cluster_history_every=4,
                     **options)
        got[name] = read_datasets(str(tmp_path / name / SW.get_folder_name(*SW.unpack(combo)) / "data" / "experiment_data.h5"))
    assert set(got["a"]) == set(got["b"]) and set(CLUSTER_DATASETS) <= set(got["a"])
    for key in CLUSTER_DATASETS + ("cluster_sizes", "Sn_final"):
        assert np.array_equal(got["a"][key], got["b"][key]), key
