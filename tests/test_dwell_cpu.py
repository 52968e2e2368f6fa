"""Host side of the strategy dwell record (no GPU): identities of the NumPy model written from the
definitions (tests/_dwell.py), dwell.host_dwell against it, the ABI (header = binding = exports,
still version 19), the option tables of the drop-in and the sweep, the datasets write_datasets
writes, and the built kernels' resources.  Every comparison is of integers and exact."""
import ctypes
import os
import re

import numpy as np
import pytest

from spgg_amd import _lib, dwell, records, spgg
from spgg_amd.h5io import read_datasets

from tests import _dwell as M
from tests._golden import Case

HEADER = os.path.join(os.path.dirname(_lib.PKG_DIR), "include", "spgg_abi.h")
NEW = ("spgg_dwell_bind", "spgg_dwell_reset", "spgg_dwell_record", "spgg_dwell_fields")


@pytest.mark.parametrize("n, m, seed", [(1, 1, 0), (7, 2, 1), (169, 9, 2), (576, 40, 3)])
def test_model_identities(n, m, seed):
    planes = M.random_planes(n, m, seed)
    first = M.row(planes[:1])   # t = t_ref
    assert first[M.NEVER] == first[M.SAME] == n
    assert first[M.NEVER_C] == first[M.BOTH_C] == first[M.NCOOP] == np.sum(planes[0] == 0)
    assert first[M.FLIPS] == 0 and first[M.COOP_TIME] == first[M.NCOOP]
    ages = first[M.AGE0:].reshape(2, M.AGE_BINS)
    assert ages[:, 0].sum() == n and ages[:, 1:].sum() == 0   # every age is 0: bin 0
    never = n
    for k in range(1, m + 1):
        r = M.row(planes[:k])
        assert r[M.NEVER] <= never and r[M.NEVER] <= r[M.SAME]
        never = r[M.NEVER]
        ages = r[M.AGE0:].reshape(2, M.AGE_BINS)
        assert ages[0].sum() == r[M.NCOOP] and ages.sum() == n
        assert r[M.NEVER_C] <= r[M.BOTH_C] <= r[M.NCOOP]
        assert r[M.COOP_TIME] == sum(int(np.sum(p == 0)) for p in planes[:k])
        f = M.fields(planes[:k])
        assert np.all(f[1] <= k - 1) and np.all(f[2] <= k)
        assert np.all(f[1][f[0] == 0] == k - 1)   # never flipped: as old as the record


def test_age_bins():
    edges = dwell.age_bin_edges()
    assert edges.dtype == np.int64 and len(edges) == dwell.DWELL_AGE_BINS + 1 == 28
    assert dwell.DWELL_SLOTS == 61 == M.SLOTS == _lib.DWELL_SLOTS
    for b in range(0, 27):
        assert M.bin_of(2 ** b - 1) == b == dwell.age_bin(2 ** b - 1) and edges[b] == 2 ** b - 1
        if b:
            assert M.bin_of(2 ** b - 2) == b - 1 == dwell.age_bin(2 ** b - 2)
    assert M.bin_of(2 ** 26 - 1) == 26   # the largest age + 1 = 2^26: spgg_create's bound on iterations
    ages = np.arange(0, 5000)
    assert np.array_equal(dwell.age_bin(ages), [M.bin_of(a) for a in ages])


@pytest.mark.parametrize("shape, m, t_ref, seed", [((1,), 1, 1, 0), ((5, 5), 3, 1, 1), ((13, 13), 12, 4, 2),
                                                   ((24, 24), 33, 17, 3)])
def test_host_dwell_equals_the_model(shape, m, t_ref, seed):
    n = int(np.prod(shape))
    planes = [p.reshape(shape) | (2 * (p.reshape(shape) ^ 1)) for p in M.random_planes(n, m, seed)]   # bit 1: ignored
    for k in range(1, m + 1):
        row, f = dwell.host_dwell(planes[:k], t_ref)
        assert row.dtype == np.int64 and row.shape == (61,) and f.shape == (3,) + shape
        assert np.array_equal(row, M.row(planes[:k])), k
        assert np.array_equal(f.reshape(3, -1), M.fields(planes[:k])), k
    assert dwell.persistence(3, 12) == 0.25 and dwell.autocorrelation(9, 12) == 0.5
    assert dwell.autocorrelation(0, 12) == -1.0 and dwell.autocorrelation(12, 12) == 1.0
    with pytest.raises(ValueError):
        dwell.host_dwell([])


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(spgg_\w+)\s*\(", src, flags=re.M))


def test_abi_still_v19_with_the_four_entry_points():
    header = open(HEADER).read()
    assert set(NEW) <= _declared(HEADER) == set(_lib.EXPORTED)
    assert int(re.search(r"#define SPGG_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 19
    assert int(re.search(r"#define SPGG_DWELL_SLOTS (\d+)", header).group(1)) == _lib.DWELL_SLOTS == 61
    assert int(re.search(r"#define SPGG_DWELL_AGE_BINS (\d+)", header).group(1)) == _lib.DWELL_AGE_BINS == 27
    enum = dict(re.findall(r"SPGG_DW_(\w+) = (\d+)", header))
    assert {k: int(v) for k, v in enum.items()} == dict(NEVER=M.NEVER, NEVER_C=M.NEVER_C, SAME=M.SAME, BOTH_C=M.BOTH_C,
                                                         NCOOP=M.NCOOP, FLIPS=M.FLIPS, COOP_TIME=M.COOP_TIME, AGE0=M.AGE0)
    assert (_lib.DW_NEVER, _lib.DW_NEVER_C, _lib.DW_SAME, _lib.DW_BOTH_C, _lib.DW_NCOOP, _lib.DW_FLIPS,
            _lib.DW_COOP_TIME, _lib.DW_AGE0) == tuple(range(8))
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    assert lib.spgg_abi_version() == 19 and all(hasattr(lib, name) for name in NEW)
    out = (ctypes.c_int64 * 64)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert lib.spgg_dwell_bind(None, p, p) == _lib.E_ARG
    assert lib.spgg_dwell_reset(None, 1, None) == _lib.E_ARG
    assert lib.spgg_dwell_record(None, 1, p, 64, None) == _lib.E_ARG
    assert lib.spgg_dwell_fields(None, 1, p, 64, None) == _lib.E_ARG
    assert not any(out)


def test_option_tables():
    """The dwell options through the one entry point (the table itself: tests/test_records_cpu.py)."""
    def values(**v):
        run_kw, extras = spgg.record_options(v)
        return run_kw["dwell_every"], extras["dwell_fields"]

    assert spgg.SPGG.dwell_history_every == 0 and spgg.SPGG.dwell_fields is False
    assert issubclass(dwell.Dwell, records.Record) and records.KINDS["dwell"] is dwell.Dwell
    assert values() == (0, False)
    assert values(dwell_history_every="4", dwell_fields=1) == (4, True)
    assert values(dwell_history_every=None) == (0, False)
    with pytest.raises(ValueError, match="dwell_fields needs dwell_history_every > 0"):
        values(dwell_fields=True)
    rec = dwell.Dwell(7, 3, 40)
    assert (rec.every, rec.t0, rec.rows, rec.key) == (7, 3, 6, (7,)) and rec.iters(20).tolist() == [3, 10, 17]


def test_sweep_pops_the_options(tmp_path, monkeypatch):
    from spgg_amd import engine as E
    from spgg_amd import sweep as SW
    monkeypatch.chdir(tmp_path)
    params = (3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning")
    seen = {}

    class FakeSPGG:
        rep_avg_history = []
        dwell_history_every, dwell_fields = 0, False

        def __init__(self, **kw):
            assert not {k for k in kw if k.startswith("dwell")}, kw
            seen["ctor"] = kw

        def run(self, filename):
            seen["attrs"] = (self.dwell_history_every, self.dwell_fields, self.reputation_history_every)
            return 0.5, 0.5, None

    monkeypatch.setattr(spgg, "SPGG", FakeSPGG)
    SW.run_one_experiment(params, L=8, iterations=3, dwell_history_every=5, dwell_fields=True)
    assert seen["attrs"] == (5, True, 0) and seen["ctor"]["L"] == 8
    SW.run_one_experiment(params, L=8, iterations=3)
    assert seen["attrs"] == (0, False, 0)
    kw = dict(L=8, dwell_history_every=2)
    got = SW.pop_record_options(kw)
    assert (got["dwell_history_every"], got["dwell_fields"]) == (2, False) and kw == dict(L=8)

    class FakeEngine:
        def __init__(self, L, iterations, replicas, **kw):
            self.L, self.R = L, len(replicas)
            self.snapshots = [dict() for _ in replicas]
            self.png_frames = [dict() for _ in replicas]

        def run(self, **kw):
            seen["run"] = kw

        def histories(self):
            return [dict() for _ in range(self.R)]

        def dwell_histories(self):
            return [dict(marker=k) for k in range(self.R)]

        def dwell_fields(self, k):
            return dict(flip_count=k, strategy_age=10 + k, cooperation_frequency=0.5)

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
                 dwell_history_every=2, dwell_fields=True)
    assert seen["run"]["dwell_every"] == 2 and seen["run"]["reputation_every"] == 0
    assert [w["records"]["dwell"] for w in written] == [
        dict(marker=k, flip_count_final=k, strategy_age_final=10 + k, cooperation_frequency_final=0.5) for k in (0, 1)]
    written.clear()
    SW.run_batch([params], seeds=[1], save_png=False, verbose=False, L=8, iterations=3, dwell_history_every=3)
    assert written[0]["records"]["dwell"] == dict(marker=0)
    written.clear()
    SW.run_batch([params], seeds=[1], save_png=False, verbose=False, L=8, iterations=3)
    assert seen["run"]["dwell_every"] == 0 and written[0]["records"]["dwell"] is None


def test_write_datasets_takes_the_dwell_record(tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", "npz")
    c = Case("m1_rep_L16")
    L = c.kwargs["L"]
    snaps = {int(k[11:]): (c.datasets[k], c.datasets["Sn_snapshot_" + k[11:]])
             for k in c.datasets if k.startswith("R_snapshot_")}

    def write(name, **kw):
        fn = str(tmp_path / name)
        spgg.write_datasets(fn, c.datasets, snaps, c.Sn, c.R, c.kwargs.get("R_min", -10), c.kwargs.get("R_max", 10),
                            spgg.track_positions(L), **kw)
        return read_datasets(fn)

    planes = [p.reshape(L, L) for p in M.random_planes(L * L, 11, 5)]
    its = np.array([1, 6, 11])
    rows = np.stack([dwell.host_dwell(planes[:t], 1)[0] for t in its]).astype(np.int32)
    rec = dwell.Dwell(5, 1, 11)
    hist = rec.datasets(None, 0, its, rows.astype(np.int64))
    assert tuple(hist) == dwell.DWELL_DATASETS
    f = dwell.host_dwell(planes, 1)[1]
    final = dict(flip_count_final=f[0].astype(np.int32), strategy_age_final=f[1].astype(np.int32),
                 cooperation_frequency_final=f[2] / np.float64(11))
    assert tuple(final) == dwell.DWELL_FIELD_DATASETS
    base = write("b.npz")
    assert sorted(base) == sorted(c.datasets)
    got = write("a.npz", records=dict(dwell=hist))
    assert set(got) - set(base) == set(hist)
    got = write("c.npz", records=dict(dwell=dict(hist, **final)))
    assert set(got) - set(base) == set(hist) | set(final)
    shapes = dict(dwell_history_iters=(3,), dwell_ref_iteration=(), persistence_history=(3, 2),
                  autocorrelation_history=(3, 3), flip_total_history=(3,), cooperator_time_history=(3,),
                  strategy_age_hist_history=(3, 2, 27), flip_count_final=(L, L), strategy_age_final=(L, L),
                  cooperation_frequency_final=(L, L))
    for k, v in dict(hist, **final).items():
        want = np.float64 if k == "cooperation_frequency_final" else np.int64
        assert got[k].dtype == want and got[k].shape == shapes[k] and np.array_equal(got[k], v), k
    assert got["dwell_ref_iteration"] == 1
    assert np.array_equal(got["persistence_history"][:, 0], rows[:, M.NEVER])
    assert np.array_equal(got["autocorrelation_history"], rows[:, [M.SAME, M.BOTH_C, M.NCOOP]])
    assert np.array_equal(got["strategy_age_hist_history"].reshape(3, -1), rows[:, M.AGE0:])


def test_kernel_resources():
    """The six dwell kernels (reset, the step launch's dword and byte instances, zero, record,
    fields) use no scratch and spill nothing; none carries the reputation kernels' name."""
    from tests.test_kernel_resources_cpu import LIB, READELF, _kernels
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    mine = {k: v for k, v in _kernels(LIB).items() if "spgg_dwell_" in k}
    assert len(mine) == 6 and len([k for k in mine if "spgg_dwell_step_kernel" in k]) == 2, sorted(mine)
    for part in ("reset_kernel", "zero_kernel", "record_kernel", "fields_kernel"):
        assert len([k for k in mine if f"spgg_dwell_{part}" in k]) == 1, part
    for name, f in mine.items():
        assert "spgg_reputation_" not in name
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, name
        assert f["vgpr_count"] <= 64, (name, f["vgpr_count"])   # eight waves per SIMD
