"""What the three in-run records share (records.Record, BatchEngine.run): a record started at a
later iteration holds t0, t0 + k, ... in one row each, and a run continued with the same settings
keeps the record object and its tensors.  Expected values: the host models of tests/_clusters.py,
_correlations.py and _reputation.py on the planes of an engine stepped one iteration at a time."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")
pytestmark = pytest.mark.gpu

from spgg_amd.engine import BatchEngine  # noqa: E402

from tests import _clusters as KC  # noqa: E402
from tests.test_gpu_correlations import _assert_histories as assert_correlations  # noqa: E402
from tests.test_gpu_reputation import _assert_histories as assert_reputation  # noqa: E402
from tests.test_gpu_reputation import _params, _stepwise_expectation  # noqa: E402

L, T, EVERY, T0, D = 16, 30, 4, 6, 3
CASES = {"clusters": (dict(clusters_every=EVERY), "cluster_histories"),
         "correlations": (dict(correlations_every=EVERY, correlations_max_d=D), "correlation_histories"),
         "reputation": (dict(reputation_every=EVERY, reputation_max_d=D), "reputation_histories")}


def _make():
    return BatchEngine(L, T, [_params(seed=s) for s in (5, 6)], use_second_order=False, rng="mt19937")


@pytest.fixture(scope="module")
def stepwise():
    """([replica][t] -> (S_t, R_t)), last iteration per replica: computed once for the three cases."""
    return _stepwise_expectation(_make, T)


@pytest.mark.parametrize("kind", sorted(CASES))
def test_record_from_a_later_iteration_and_continued(kind, stepwise):
    planes, last = stepwise
    kw, getter = CASES[kind]
    eng = _make()
    try:
        eng.step(T0 - 1)
        eng.run(snapshots=False, **kw)
        record = eng.records[kind]
        out = list(record.out)
        assert record.t0 == T0 and out and all(o.shape[1] == (T - T0) // EVERY + 1 for o in out)
        first = getattr(eng, getter)()
        eng.run(snapshots=False, **kw)   # the run is over: nothing is added
        assert eng.records[kind] is record and len(record.out) == len(out)
        assert all(a is b for a, b in zip(record.out, out))
        hist = getattr(eng, getter)()
    finally:
        eng.close()
    S = [{t: p[0] for t, p in rep.items()} for rep in planes]
    if kind == "clusters":
        for k, h in enumerate(hist):
            its = np.arange(T0, last[k] + 1, EVERY)
            assert np.array_equal(h["cluster_history_iters"], its), k
            want = np.array([KC.expected_record(S[k][t], False) for t in its], dtype=np.int64).reshape(-1, 3)
            for j, key in enumerate(("cluster_count_history", "largest_cluster_history", "cd_bond_history")):
                assert h[key].dtype == np.int64 and np.array_equal(h[key], want[:, j]), (k, key)
    elif kind == "correlations":
        assert_correlations(hist, S, last, EVERY, D, t0=T0)
    else:
        assert_reputation(hist, planes, last, EVERY, 20, D, t0=T0)
    for a, b in zip(first, hist):
        assert set(a) == set(b) and all(np.array_equal(a[key], b[key]) for key in a)
