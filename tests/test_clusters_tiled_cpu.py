"""Host side of the tiled device cluster labelling (spgg_clusters_tiled; no GPU): the NumPy model of
the shipped scheme (tests/_clusters_tiled.py) against scipy's labelling, the device caps against what
the model needs at side 1000, the ABI (header = binding = exports, still version 19), the built
kernels' resources, the option tables and the validation of clusters_tiled.  Every comparison is of
integers and exact."""
import ctypes
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

pytest.importorskip("scipy")

from spgg_amd import _lib, records, spgg, sweep  # noqa: E402

from tests import _clusters as K  # noqa: E402
from tests import _clusters_tiled as M  # noqa: E402

HEADER = os.path.join(os.path.dirname(_lib.PKG_DIR), "include", "spgg_abi.h")
NEW = ("spgg_clusters_tiled", "spgg_clusters_tiled_workspace")
LDS_LIMIT = 163840   # bytes one gfx950 workgroup may declare


def _check(mask, periodic, tile):
    sizes, rec, stats = M.model(mask, periodic, tile)
    want = K.expected_sizes(mask, periodic)
    assert np.array_equal(sizes[sizes > 0], want)
    assert not np.any(sizes[~np.asarray(mask, dtype=bool).ravel()])
    assert rec == K.expected_record(np.where(mask, 0, 1), periodic)
    return stats


@pytest.mark.parametrize("L", [1, 2, 3, 5, 13, 16, 33, 64])
def test_model_equals_scipy(L):
    for name, mask in K.pattern_masks(L, seed=L):
        for tile in (8, 16, 200):
            for periodic in (False, True):
                stats = _check(mask, periodic, tile)
                assert 4 * stats["passes"] <= _lib.CLUSTERS_MAX_PASSES, (name, tile, periodic, stats)


def test_representatives_are_smallest_raster_indices():
    L = 33
    from scipy.ndimage import label
    mask = K.random_mask(L, 0.593, 5)
    sizes, _rec, _ = M.model(mask, False, 8)
    lab, k = label(mask)
    first = [int(np.flatnonzero(lab.ravel() == j)[0]) for j in range(1, k + 1)]
    assert np.flatnonzero(sizes).tolist() == first


def _side_1000_masks():
    L = 1000
    s = K.serpentines(L)
    named = [("spiral", K.spiral(L))] + [(f"serpentine{k}", m) for k, m in enumerate(s)]
    named += [("random0.55", K.random_mask(L, 0.55, 1)), ("random0.593", K.random_mask(L, 0.593, 2)),
              ("random0.7", K.random_mask(L, 0.7, 3)), ("all_c", np.ones((L, L), dtype=bool))]
    return named


def test_model_at_side_1000_and_the_caps():
    """The library's tile on a cfg5 lattice: scipy's result, and every device cap (a tile's passes, a
    root walk's n steps, a union's retries) at least 4 x what the lock-step model needs."""
    n = 1000 * 1000
    worst = dict(passes=0, walk=0, retries=0)
    for name, mask in _side_1000_masks():
        stats = _check(mask, name != "random0.55", _lib.CLUSTERS_TILE_DEFAULT)   # both boundary modes occur
        print(name, stats)
        for key in worst:
            worst[key] = max(worst[key], stats[key])
    assert 4 * worst["passes"] <= _lib.CLUSTERS_MAX_PASSES, worst
    assert 4 * worst["walk"] <= n, worst
    assert 4 * worst["retries"] <= _lib.CLUSTERS_TILED_MAX_RETRIES, worst


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(spgg_\w+)\s*\(", src, flags=re.M))


def test_abi_still_v19_with_the_two_entry_points():
    header = open(HEADER).read()
    assert set(NEW) <= _declared(HEADER) == set(_lib.EXPORTED)
    assert int(re.search(r"#define SPGG_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 19
    assert int(re.search(r"#define SPGG_CLUSTERS_TILED_MAX_RETRIES (\d+)", header).group(1)) == \
        _lib.CLUSTERS_TILED_MAX_RETRIES
    assert (_lib.CLUSTERS_TILE_MIN, _lib.CLUSTERS_TILE_MAX) == (M.TILE_MIN, M.TILE_MAX) == (8, 200)
    assert M.TILE_MIN <= _lib.CLUSTERS_TILE_DEFAULT <= M.TILE_MAX
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    assert lib.spgg_abi_version() == 19 and all(hasattr(lib, name) for name in NEW)
    out = (ctypes.c_int32 * 8)()
    p = ctypes.cast(out, ctypes.c_void_p)
    words = ctypes.c_int64(-1)
    assert lib.spgg_clusters_tiled_workspace(None, ctypes.byref(words)) == _lib.E_ARG and words.value == -1
    assert lib.spgg_clusters_tiled(None, 1, 0, 0, p, None, p, 3, None) == _lib.E_ARG
    assert not any(out)


def _tiled_kernels(path):
    """{kernel symbol: metadata fields} of the tiled labelling's kernels from the code objects' notes."""
    from tests.test_kernel_resources_cpu import READELF, _code_objects
    fields = ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(_code_objects(path)):
            f = os.path.join(tmp, f"co{i}.o")
            open(f, "wb").write(co)
            notes = subprocess.run([READELF, "--notes", f], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "spgg_clusters_tiled_" in name:
                    res[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in fields}
    return res


def test_kernel_resources():
    """The tiled labelling's kernels (init, the tile pass's four LDS instances, seam, count, record) use
    no scratch, spill nothing and declare at most 160 KiB of LDS."""
    from tests.test_kernel_resources_cpu import LIB, READELF
    if not os.path.exists(LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available")
    mine = _tiled_kernels(LIB)
    assert len(mine) == 8 and len([k for k in mine if "tile_kernel" in k]) == 4, sorted(mine)
    for part in ("init_kernel", "seam_kernel", "count_kernel", "record_kernel"):
        assert len([k for k in mine if f"spgg_clusters_tiled_{part}" in k]) == 1, part
    for name, f in mine.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, name
        assert f["group_segment_fixed_size"] <= LDS_LIMIT, (name, f)
    lds = sorted(f["group_segment_fixed_size"] for k, f in mine.items() if "tile_kernel" in k)
    assert lds == [4 * s * s + 32 for s in (32, 64, 128, 200)], lds   # two 16-bit planes and eight shared words


def test_option_tables():
    """The tiled option through the one entry point: an option of the clusters kind (the table itself:
    tests/test_records_cpu.py)."""
    assert [o[0] for o in records.Clusters.options][2] == "cluster_history_tiled"
    assert spgg.SPGG.cluster_history_tiled is False
    assert spgg.record_options({})[0]["clusters_tiled"] is False
    assert spgg.record_options({"cluster_history_tiled": True})[0]["clusters_tiled"] is True
    assert spgg.record_options({"cluster_history_tiled": 8})[0]["clusters_tiled"] == 8
    kw = dict(L=16, cluster_history_tiled=16, cluster_history_every=5)
    got = sweep.pop_record_options(kw)
    assert (got["cluster_history_tiled"], got["cluster_history_every"]) == (16, 5) and kw == dict(L=16)
    assert sweep.pop_record_options({})["cluster_history_tiled"] is False


def test_validation_of_clusters_tiled():
    """Clusters.validate: the tile's range, clusters_tiled without clusters_every, and the key; the
    refusal above side 200 without the option still names the side."""
    small, wide = types.SimpleNamespace(L=24, clusters_max_side=200), types.SimpleNamespace(L=1000, clusters_max_side=200)
    V = records.Clusters.validate
    assert V(small, 3, False) == (3, False, None) == V(small, 3, False, False)
    assert V(small, 3, True, True) == (3, True, 0)
    assert V(wide, 2, False, 64) == (2, False, 64)
    assert V(wide, 1, False, 8)[2] == 8 and V(wide, 1, False, 200)[2] == 200
    assert V(small, 0, False) == (0, False, None)
    for tiled in (True, 8):
        with pytest.raises(ValueError, match="clusters_every"):
            V(small, 0, False, tiled)
    for tile in (7, 201, 1, -8):
        with pytest.raises(ValueError, match="8 .. 200"):
            V(wide, 1, False, tile)
    with pytest.raises(ValueError, match="200") as e:
        V(wide, 1, False)
    assert "clusters_tiled" in str(e.value)
    assert "pass cap (32)" in records.clusters_cap_text(False)
    assert "retry cap (256)" not in records.clusters_cap_text(False)
    assert "retry cap 256" in records.clusters_cap_text(True) and records.clusters_cap_text(True) != records.clusters_cap_text(False)
