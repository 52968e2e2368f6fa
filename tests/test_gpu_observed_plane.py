"""Which of the two planes an observer reads (csrc/spgg_observe.h: observed_iter / observed_plane),
with planes that differ.  The other observer tests meet absorbed replicas only where both planes
hold the same lattice; here every replica holds two different random lattices and two different
reputation fields, stop_iter marks a live replica, one absorbed at an odd iteration, one at an even
one and one at the first of the two observed iterations, and every observer must return the host's
value for plane (tt - 1) & 1, tt by the rule of include/spgg_abi.h restated below.  Integers, exact.  (The
dwell read-outs clamp at their t_ref and need a tracked run: tests/test_gpu_dwell.py
::test_a_replica_that_absorbs_mid_run.)"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")

from spgg_amd.engine import BatchEngine, InitState  # noqa: E402
from spgg_amd.records import host_pair_counts, host_reputation_pair_sums, reputation_bin_edges  # noqa: E402

from tests import _clusters as K  # noqa: E402
from tests.test_gpu_clusters import _params  # noqa: E402

L, T, BINS = 5, 8, 20   # odd L: replica planes at odd byte offsets
TILE = 8                # the smallest tile; with wrap the lattice edge is a seam: the seam launch reads the plane too
STOPS = (0, 3, 4, 6)
TIMES = (6, 7)
BOUNDS = dict(R_min=-128, R_max=127)   # int8 reputation at unit 1


def observed_plane_index(stop, t):
    """spgg_abi.h: S_t is read from S[(t-1) & 1]; a replica absorbed at s < t (stop_iter = s != 0)
    keeps its state in S[(s-1) & 1]."""
    tt = stop if stop != 0 and stop < t else t
    return (tt - 1) & 1


def _lattices(seed=20):
    """S [2][R][L][L] uint8 with dirty bits 1-4, Rep [2][R][L][L] int8: the two planes of every replica differ."""
    rs = np.random.RandomState(seed)
    R = len(STOPS)
    S = ((rs.rand(2, R, L, L) < 0.45).astype(np.uint8) | (rs.randint(0, 16, (2, R, L, L)) << 1)).astype(np.uint8)
    Rep = rs.randint(-128, 128, (2, R, L, L)).astype(np.int8)
    return S, Rep


def _host(S, Rep):
    """Every observable of one replica's plane, as a dict of integer arrays."""
    coop = (S & 1) == 0
    x = Rep.astype(np.float64)
    e = reputation_bin_edges(BOUNDS["R_min"], BOUNDS["R_max"], BINS)
    s, rows, cols = host_reputation_pair_sums(Rep)
    return dict(walls=np.array(K.expected_record(S, False)), periodic=np.array(K.expected_record(S, True)),
                pairs=host_pair_counts(S).reshape(-1),
                hist=np.concatenate([np.histogram(x[coop], bins=e)[0], np.histogram(x[~coop], bins=e)[0]]),
                rep_pairs=np.concatenate([[s], rows, cols]))


def test_the_host_values_tell_the_planes_apart():
    """Otherwise the device test below could not fail (CPU: no GPU is touched)."""
    S, Rep = _lattices()
    for k in range(len(STOPS)):
        a, b = _host(S[0, k], Rep[0, k]), _host(S[1, k], Rep[1, k])
        for key in a:
            assert not np.array_equal(a[key], b[key]), (k, key)
    planes = {(s, t): observed_plane_index(s, t) for s in STOPS for t in TIMES}
    assert planes == {(0, 6): 1, (3, 6): 0, (4, 6): 1, (6, 6): 1, (0, 7): 0, (3, 7): 0, (4, 7): 1, (6, 7): 1}


@pytest.mark.gpu
def test_every_observer_reads_the_plane_of_the_observed_iteration():
    S, Rep = _lattices()
    R, D = len(STOPS), L // 2
    init = [InitState(Q=np.zeros((L, L, 2, 2)), S=S[0, k]) for k in range(R)]
    eng = BatchEngine(L, T, [_params(seed=k, **BOUNDS) for k in range(R)], use_second_order=False, rng="philox",
                      init=init)
    try:
        assert eng.rep_int8 and np.all(eng.rep_units == 1.0)
        torch.cuda.synchronize()
        eng.S.copy_(torch.from_numpy(S.reshape(2, R, L * L)).to(eng.dev))
        eng.Rep.copy_(torch.from_numpy(Rep.reshape(2, R, L * L)).to(eng.dev))
        eng.stop_iter.copy_(torch.tensor(STOPS, dtype=torch.int32).to(eng.dev))
        torch.cuda.synchronize()   # the observers run on the groups' streams

        lib = eng.lib
        calls = dict(walls=(lib.spgg_clusters, (0, None), 3, torch.int32),
                     periodic=(lib.spgg_clusters, (1, None), 3, torch.int32),
                     tiled_walls=(lib.spgg_clusters_tiled, (0, TILE, eng._clusters_workspace(), None), 3, torch.int32),
                     tiled_periodic=(lib.spgg_clusters_tiled, (1, TILE, eng._clusters_workspace(), None), 3, torch.int32),
                     pairs=(lib.spgg_correlations, (D,), 2 * (D + 1), torch.int32),
                     hist=(lib.spgg_reputation_hist, (BINS, eng._reputation_edges(BINS)), 2 * BINS, torch.int32),
                     rep_pairs=(lib.spgg_reputation_pairs, (D,), 2 * (D + 1) + 1, torch.int64))
        host = [[_host(S[p, k], Rep[p, k]) for k in range(R)] for p in range(2)]
        for t in TIMES:
            for name, (fn, args, width, dtype) in calls.items():
                out = torch.zeros((R, width), dtype=dtype, device=eng.dev)
                eng._observe(fn, t, args, out)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                key = name.replace("tiled_", "")
                for k, stop in enumerate(STOPS):
                    p = observed_plane_index(stop, t)
                    print(t, name, k, p, got[k].tolist())
                    assert np.array_equal(got[k], host[p][k][key]), (t, name, k, p, got[k], host[p][k][key])
    finally:
        eng.close()
