"""Host side of the device pair counts (no GPU): the NumPy model of the kernel's packed cyclic
rotation against np.roll, engine.host_pair_counts against this suite's own expectation, the two
host helpers on hand-built inputs, the new entry points' null-argument errors, the sweep's
handling of the two overrides and write_datasets' optional datasets."""
import ctypes
import math
import os

import numpy as np
import pytest

from spgg_amd import _lib, spgg
from spgg_amd.engine import correlation_function, correlation_length, host_pair_counts
from spgg_amd.h5io import read_datasets

from tests import _correlations as K
from tests._golden import Case

SIDES = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 96, 127, 129, 200]


@pytest.mark.parametrize("L", SIDES)
def test_rotation_model_equals_roll(L):
    """The kernel's rotation of an L-bit row stored in 32-bit words, for every d <= L // 2: d across
    word boundaries, d >= 32, the wrap at bit L inside a word, one-word and two-word rows."""
    rs = np.random.RandomState(L)
    for p in (0.5, 0.1):
        mask = rs.rand(L, L) < p
        assert np.array_equal(K.unpack(K.pack(mask), L), mask)
        for d in range(L // 2 + 1):
            assert np.array_equal(K.model_rotate(mask, d), np.roll(mask, -d, axis=1)), (L, p, d)


@pytest.mark.parametrize("L", [1, 2, 3, 5, 31, 33, 64, 65])
def test_count_model_equals_expectation(L):
    for name, mask in K.pattern_masks(L):
        D = L // 2
        assert np.array_equal(K.model_pair_counts(mask, D), K.expected_pair_counts(mask, D)), (L, name)


def test_host_pair_counts():
    for L in (1, 2, 3, 5, 33, 64):
        names, planes = K.planes_of(L)
        for name, S in zip(names, planes):
            mask = (S & 1) == 0
            for max_d in (None, 0, 1):
                if max_d is not None and max_d > L // 2:
                    continue
                D = L // 2 if max_d is None else max_d
                got = host_pair_counts(S, max_d)
                assert got.dtype == np.int64 and got.shape == (2, D + 1), (L, name, max_d)
                assert np.array_equal(got, K.expected_pair_counts(mask, D)), (L, name, max_d)
                assert got[0, 0] == got[1, 0] == int(mask.sum())
    with pytest.raises(ValueError):
        host_pair_counts(np.zeros((6, 6), dtype=np.uint8), 4)
    with pytest.raises(ValueError):
        host_pair_counts(np.zeros((6, 6), dtype=np.uint8), -1)


def test_correlation_function_and_length():
    L = 12
    n = L * L
    pc = K.expected_pair_counts(np.ones((L, L), dtype=bool), L // 2)     # all-C: an absorbed lattice
    G = correlation_function(pc[0], pc[1], n)
    assert G.shape == (L // 2 + 1,) and np.all(G == 0.0)
    assert math.isnan(correlation_length(G))
    # the definition, on a random lattice: <c c_d> averaged over the two directions, minus rho^2
    mask = np.random.RandomState(4).rand(L, L) < 0.4
    pc = K.expected_pair_counts(mask, L // 2)
    G = correlation_function(pc[0], pc[1], n)
    rho = mask.mean()
    for d in range(L // 2 + 1):
        want = 0.5 * ((mask & np.roll(mask, -d, 1)).mean() + (mask & np.roll(mask, -d, 0)).mean()) - rho * rho
        assert abs(G[d] - want) < 1e-15, d
    assert abs(G[0] - rho * (1 - rho)) < 1e-15
    # leading axes (a history): the distance is the last axis
    Gh = correlation_function(np.stack([pc[0], pc[0]]), np.stack([pc[1], pc[1]]), n)
    assert Gh.shape == (2, L // 2 + 1) and np.array_equal(Gh[1], G)
    # a G that never decays
    assert correlation_length(np.ones(8)) == math.inf
    assert correlation_length(np.array([2.0, 1.9, 1.8])) == math.inf
    # geometric G = q^d: the first d with q^d <= 1/e, interpolated linearly between d - 1 and d
    for q in (0.9, 0.5, 0.3, math.exp(-0.5)):
        G = 3.0 * q ** np.arange(40)
        d = next(k for k in range(1, 40) if q ** k <= 1 / math.e)
        want = d - 1 + (q ** (d - 1) - 1 / math.e) / (q ** (d - 1) - q ** d)
        got = correlation_length(G)
        assert abs(got - want) < 1e-12, (q, got, want)
        assert d - 1 <= got <= d
    assert abs(correlation_length(np.array([1.0, 0.2])) - (1.0 - 1 / math.e) / 0.8) < 1e-12


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libspgg_hip.so not built")
def test_argument_errors_without_device():
    lib = _lib.load()
    side = ctypes.c_int32(-5)
    assert lib.spgg_correlations_max_side(None, ctypes.byref(side)) == _lib.E_ARG
    assert side.value == -5
    out = (ctypes.c_int32 * 4)()
    assert lib.spgg_correlations(None, 1, 1, ctypes.cast(out, ctypes.c_void_p), 4, None) == _lib.E_ARG
    assert list(out) == [0, 0, 0, 0]
    assert _lib.ABI_VERSION == lib.spgg_abi_version() >= 18


def test_kernel_resources(tmp_path):
    """Two instances, no scratch, no spills; the small one declares 8 KiB (its workgroups share a
    CU), the full one holds the supported side's packed lattice within what a workgroup may declare."""
    import re
    import subprocess
    from tests.test_kernel_resources_cpu import LIB, READELF, _code_objects
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    blocks = []
    for i, co in enumerate(_code_objects(LIB)):
        f = tmp_path / f"co{i}.o"
        f.write_bytes(co)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        blocks += [b for b in notes.split("- .agpr_count:")[1:] if "spgg_correlations_kernel" in b]
    assert len(blocks) == 2, len(blocks)

    def field(b, k):
        return int(re.search(rf"\.{k}:\s+(\d+)", b).group(1))

    lds = sorted(field(b, "group_segment_fixed_size") for b in blocks)
    assert lds[0] == 8192 and 4 * 256 * K.row_words(256) <= lds[0]
    for b in blocks:
        assert field(b, "private_segment_fixed_size") == 0
        assert field(b, "vgpr_spill_count") == 0 and field(b, "sgpr_spill_count") == 0
        assert field(b, "max_flat_workgroup_size") == 1024
    # the side the library reports is the largest whose packed lattice fits the full instance
    top = 1137   # (spgg_correlations_max_side needs a context; the GPU tests read it)
    assert 4 * top * K.row_words(top) <= lds[1] <= 163840 < 4 * (top + 1) * K.row_words(top + 1)


def test_write_datasets_takes_the_correlation_record(tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", "npz")
    c = Case("m1_rep_L16")
    snaps = {int(k[11:]): (c.datasets[k], c.datasets["Sn_snapshot_" + k[11:]])
             for k in c.datasets if k.startswith("R_snapshot_")}

    def write(name, **kw):
        fn = str(tmp_path / name)
        spgg.write_datasets(fn, c.datasets, snaps, c.Sn, c.R, c.kwargs.get("R_min", -10), c.kwargs.get("R_max", 10),
                            spgg.track_positions(c.kwargs["L"]), **kw)
        return read_datasets(fn)

    hist = dict(correlation_history_iters=np.array([1, 6]),
                pair_count_rows_history=np.arange(10, dtype=np.int32).reshape(2, 5),
                pair_count_cols_history=np.arange(10, 20).reshape(2, 5))
    assert set(spgg.CORRELATION_DATASETS) == set(hist)
    got = write("a.npz", records=dict(correlations=hist))
    base = write("b.npz")
    assert set(got) - set(base) == set(hist) and sorted(base) == sorted(c.datasets)
    for k, v in hist.items():
        assert got[k].dtype == np.int64 and np.array_equal(got[k], v), k
    assert spgg.SPGG.correlation_history_every == 0 and spgg.SPGG.correlation_max_distance is None


def test_sweep_pops_the_overrides(tmp_path, monkeypatch):
    """correlation_history_every / correlation_max_distance are class attributes of the drop-in:
    run_one_experiment and run_batch take them among the model overrides and keep them from the
    constructor (run_one_experiment) and from RUNNER_MODEL's keys (run_batch)."""
    from spgg_amd import engine as E
    from spgg_amd import sweep as SW
    monkeypatch.chdir(tmp_path)
    params = (3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning")
    seen = {}

    class FakeSPGG:
        correlation_history_every = 0
        correlation_max_distance = None
        rep_avg_history = []

        def __init__(self, **kw):
            assert not {k for k in kw if k.startswith(("correlation_", "cluster_history"))}, kw
            seen["ctor"] = kw

        def run(self, filename):
            seen["attrs"] = (self.correlation_history_every, self.correlation_max_distance,
                             self.cluster_history_every)
            return 0.5, 0.5, None

    monkeypatch.setattr(spgg, "SPGG", FakeSPGG)
    SW.run_one_experiment(params, L=8, iterations=3, correlation_history_every=5, correlation_max_distance=4)
    assert seen["attrs"] == (5, 4, 0) and seen["ctor"]["L"] == 8
    SW.run_one_experiment(params, L=8, iterations=3)
    assert seen["attrs"] == (0, None, 0)

    class FakeEngine:
        def __init__(self, L, iterations, replicas, **kw):
            self.L, self.R = L, len(replicas)
            self.snapshots = [dict() for _ in replicas]
            self.png_frames = [dict() for _ in replicas]

        def run(self, **kw):
            seen["run"] = kw

        def histories(self):
            return [dict() for _ in range(self.R)]

        def correlation_histories(self):
            seen["asked"] = True
            return [dict(marker=k) for k in range(self.R)]

        def final_state(self, k):
            return None, np.zeros((self.L, self.L)), np.ones((self.L, self.L), dtype=np.int64)

        def cluster_sizes(self, k):
            return np.zeros(0, dtype=np.int64)

        def close(self):
            pass

    written = []
    monkeypatch.setattr(E, "BatchEngine", FakeEngine)
    monkeypatch.setattr(spgg, "write_datasets", lambda *a, **kw: written.append(kw))
    SW.run_batch([params, params], seeds=[1, 2], save_png=False, verbose=False, L=8, iterations=3,
                 correlation_history_every=2, correlation_max_distance=3)
    assert seen["run"]["correlations_every"] == 2 and seen["run"]["correlations_max_d"] == 3
    assert seen["run"]["clusters_every"] == 0 and seen.pop("asked")
    assert [w["records"]["correlations"] for w in written] == [dict(marker=0), dict(marker=1)]
    written.clear()
    SW.run_batch([params], seeds=[1], save_png=False, verbose=False, L=8, iterations=3)
    assert seen["run"]["correlations_every"] == 0 and seen["run"]["correlations_max_d"] is None
    assert "asked" not in seen and written[0]["records"]["correlations"] is None
