"""Host side of the device cluster labelling (no GPU): write_datasets keeps the reference's file by
default and takes the engine's cluster arrays when given, the new entry points refuse null
arguments before any device call, and the built cluster kernel fits its resources (read from
the code object's metadata notes, as tests/test_kernel_resources_cpu.py does)."""
import ctypes
import os

import numpy as np
import pytest

from spgg_amd import _lib, spgg
from spgg_amd.engine import host_cluster_sizes
from spgg_amd.h5io import read_datasets

from tests import _clusters as K
from tests._golden import Case
from tests.test_kernel_resources_cpu import LIB, READELF, _code_objects

LDS_LIMIT = 163840   # bytes one gfx950 workgroup may declare


def _write(c, tmp_path, name, **kw):
    fn = str(tmp_path / name)
    snaps = {int(k[11:]): (c.datasets[k], c.datasets["Sn_snapshot_" + k[11:]])
             for k in c.datasets if k.startswith("R_snapshot_")}
    L = c.kwargs["L"]
    spgg.write_datasets(fn, c.datasets, snaps, c.Sn, c.R, c.kwargs.get("R_min", -10), c.kwargs.get("R_max", 10),
                        spgg.track_positions(L), **kw)
    return read_datasets(fn)


def test_write_datasets_defaults_write_the_reference_file(tmp_path, monkeypatch):
    """Names, dtypes and bytes of every dataset as the reference recorded them for this run (the
    fixture's arrays go in, the fixture's datasets come out -- cluster_sizes labelled on the host)."""
    pytest.importorskip("scipy")
    monkeypatch.setenv("SPGG_H5_SINK", "npz")
    c = Case("m1_rep_L16")
    got = _write(c, tmp_path, "a.npz")
    want = c.datasets
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and got[k].tobytes() == w.tobytes(), k


def test_write_datasets_takes_the_engine_arrays(tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", "npz")
    c = Case("m1_rep_L16")
    clusters = np.array([7, 1, 3], dtype=np.int32)   # (any integer dtype in: int64 out, as the host's)
    hist = dict(cluster_history_iters=np.array([1, 4, 7]), cluster_count_history=np.array([5, 4, 3], dtype=np.int32),
                largest_cluster_history=np.array([9, 10, 11]), cd_bond_history=np.array([40, 38, 30]))
    got = _write(c, tmp_path, "b.npz", clusters=clusters, records=dict(clusters=hist))
    assert got["cluster_sizes"].dtype == np.int64 and np.array_equal(got["cluster_sizes"], clusters)
    assert set(spgg.CLUSTER_DATASETS) == set(hist)
    for k, v in hist.items():
        assert got[k].dtype == np.int64 and np.array_equal(got[k], v), k
    base = _write(c, tmp_path, "c.npz")
    assert set(got) - set(base) == set(hist)
    empty = _write(c, tmp_path, "d.npz", clusters=np.zeros(0, dtype=np.int64))
    assert empty["cluster_sizes"].shape == (0,) and empty["cluster_sizes"].dtype == np.int64


@pytest.mark.parametrize("periodic", [False, True])
def test_host_fallback_labelling(periodic):
    """engine.host_cluster_sizes (the path above the supported side) against this suite's own
    expectation, and spgg.cluster_sizes stays the non-periodic host utility."""
    pytest.importorskip("scipy")
    for L in (1, 2, 5, 33):
        for _name, m in K.pattern_masks(L, seed=3):
            S = np.where(m, 0, 1)
            got = host_cluster_sizes(S, periodic)
            assert got.dtype == np.int64 and np.array_equal(got, K.expected_sizes(m, periodic))
            if not periodic:
                assert np.array_equal(spgg.cluster_sizes(S), got)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libspgg_hip.so not built")
def test_argument_errors_without_device():
    lib = _lib.load()
    side = ctypes.c_int32(-5)
    assert lib.spgg_clusters_max_side(None, ctypes.byref(side)) == _lib.E_ARG
    assert side.value == -5
    rec = (ctypes.c_int32 * 3)()
    assert lib.spgg_clusters(None, 1, 0, None, ctypes.cast(rec, ctypes.c_void_p), 3, None) == _lib.E_ARG
    assert list(rec) == [0, 0, 0]


def _cluster_kernel_notes():
    import subprocess
    import tempfile
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(_code_objects(LIB)):
            f = os.path.join(tmp, f"co{i}.o")
            open(f, "wb").write(co)
            notes = subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout
            out += [b for b in notes.split("- .agpr_count:")[1:] if "spgg_clusters_kernel" in b]
    return out


def test_cluster_kernel_resources():
    """No scratch, no spills (a per-thread array in scratch would make every pass a trip to
    memory), and the two label planes within what one workgroup may declare."""
    import re
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    blocks = _cluster_kernel_notes()
    assert len(blocks) == 1, len(blocks)

    def field(k):
        return int(re.search(rf"\.{k}:\s+(\d+)", blocks[0]).group(1))

    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert 4 * 200 * 200 <= field("group_segment_fixed_size") <= LDS_LIMIT
    assert field("max_flat_workgroup_size") == 1024
