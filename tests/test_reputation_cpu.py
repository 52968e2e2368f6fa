"""Host side of the reputation record (no GPU): the NumPy model of the kernel's row scheme (padded
dwords, the shifted dword built from two aligned ones, one wrap) against np.roll, the bin rule
against np.histogram, engine.host_reputation_pair_sums against a direct double loop, the int32
lane bound of csrc/spgg_reputation.h recomputed from its constants, the ABI (header = binding =
exports, version 19), the kernels' resources, and the drop-in's / sweep's handling of the three
options.  Every comparison is of integers and exact."""
import ctypes
import os
import re

import numpy as np
import pytest

from spgg_amd import _lib, spgg
from spgg_amd.engine import (correlation_length, host_reputation_pair_sums, reputation_bin_edges,
                             reputation_correlation_function)
from spgg_amd.h5io import read_datasets

from tests import _reputation as K
from tests._golden import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(os.path.dirname(_lib.PKG_DIR), "include", "spgg_abi.h")
KERNEL_HEADER = os.path.join(_lib.PKG_DIR, "csrc", "spgg_reputation.h")

# rows shorter than a dword, one partial dword, d a multiple of 4 and not, d >= 4, a wrap inside
# the first and the last dword
SIDES = [1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 33, 64, 65, 200, 201]


@pytest.mark.parametrize("L", SIDES)
def test_rotation_model_equals_roll(L):
    for name, F in zip(K.FIELD_NAMES, K.fields_of(L)):
        lat = K.pad(F)
        assert lat.shape == (L, K.row_dwords(L))
        assert np.array_equal(np.ascontiguousarray(lat).view(np.int8).reshape(L, -1)[:, :L], F)
        for d in range(L // 2 + 1):
            assert np.array_equal(K.model_rotate(F, d), np.roll(F, -d, axis=1)), (L, name, d)


@pytest.mark.parametrize("L", SIDES)
def test_pair_sum_model_equals_definition(L):
    for name, F in zip(K.FIELD_NAMES, K.fields_of(L)):
        D = L // 2
        got, want = K.model_pair_sums(F, D), K.expected_pair_sums(F, D)
        assert got[0] == want[0], (L, name)
        assert np.array_equal(got[1], want[1]), (L, name)
        assert np.array_equal(got[2], want[2]), (L, name)
    n = L * L   # the extreme magnitudes, in closed form
    s, rows, cols = K.model_pair_sums(K.fields_of(L)[0], L // 2)
    assert s == -128 * n and np.all(rows == 128 * 128 * n) and np.all(cols == 128 * 128 * n)


def test_host_pair_sums_against_a_double_loop():
    for L in (1, 2, 3, 4, 5, 6, 7):
        for name, F in zip(K.FIELD_NAMES, K.fields_of(L)):
            for max_d in (None, 0, 1):
                if max_d is not None and max_d > L // 2:
                    continue
                D = L // 2 if max_d is None else max_d
                s, rows, cols = host_reputation_pair_sums(F, max_d)
                ws, wr, wc = K.loop_pair_sums(F, D)
                assert rows.dtype == np.int64 and cols.dtype == np.int64 and rows.shape == cols.shape == (D + 1,)
                assert int(s) == ws and np.array_equal(rows, wr) and np.array_equal(cols, wc), (L, name, max_d)
    # float input: the same sums in f64 (here of small integers, so still exact)
    F = K.fields_of(6)[6]
    s, rows, cols = host_reputation_pair_sums(F.astype(np.float64) * 0.5)
    ws, wr, wc = K.loop_pair_sums(F, 3)
    assert rows.dtype == np.float64 and s == ws * 0.5
    assert np.array_equal(rows, wr * 0.25) and np.array_equal(cols, wc * 0.25)
    with pytest.raises(ValueError):
        host_reputation_pair_sums(np.zeros((6, 6), dtype=np.int8), 4)
    with pytest.raises(ValueError):
        host_reputation_pair_sums(np.zeros((6, 6), dtype=np.int8), -1)


RANGES = [(-10, 10, 20), (-128, 127, 20), (-5.5, 3.25, 20), (-0.7, 0.9, 20), (-1, 1, 7), (-10, 10, 64),
          (-128, 127, 256), (-10, 10, 256)]


@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_bin_rule_equals_np_histogram(lo, hi, bins):
    """Dyadic and non-dyadic ranges: every edge, its two neighbouring doubles, every int8 level of
    the dyadic units that can represent the range, values outside the range."""
    edges = K.edges_of(lo, hi, bins)
    assert np.array_equal(edges, reputation_bin_edges(lo, hi, bins)) and len(edges) == bins + 1
    values = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                             np.arange(-128, 128) * 1.0, np.arange(-128, 128) * 0.25, np.arange(-128, 128) / 1024.0,
                             [lo - 1.0, hi + 1.0]])
    for x in values:   # one at a time: the bin of each value, not only the totals
        want = np.histogram([x], bins=bins, range=(lo, hi))[0]
        b = K.model_bin(edges, x)
        got = np.zeros(bins, dtype=np.int64)
        if b >= 0:
            got[b] = 1
        assert np.array_equal(got, want), (lo, hi, bins, x)
    assert np.array_equal(K.model_hist(edges, values), np.histogram(values, bins=bins, range=(lo, hi))[0])


def test_reputation_correlation_function():
    L = 12
    n = L * L
    F = K.fields_of(L)[6]
    unit = 0.25
    s, rows, cols = K.expected_pair_sums(F, L // 2)
    G = reputation_correlation_function(s, rows, cols, n, unit)
    X = F.astype(np.float64) * unit
    for d in range(L // 2 + 1):
        want = 0.5 * ((X * np.roll(X, -d, 1)).mean() + (X * np.roll(X, -d, 0)).mean()) - X.mean() ** 2
        assert abs(G[d] - want) < 1e-9 * unit * unit * 128 * 128, d
    assert abs(G[0] - X.var()) < 1e-9 * unit * unit * 128 * 128
    # leading axes (a history): the distance is the last axis, the sum has none
    Gh = reputation_correlation_function(np.array([s, s]), np.stack([rows, rows]), np.stack([cols, cols]), n, unit)
    assert Gh.shape == (2, L // 2 + 1) and np.array_equal(Gh[1], G)
    assert isinstance(correlation_length(G), float)   # reused as it stands
    flat = K.expected_pair_sums(np.full((L, L), 5, dtype=np.int8), L // 2)
    assert np.all(reputation_correlation_function(*flat, n, 1.0) == 0.0)


def _constant(src, name):
    m = re.search(rf"constexpr\s+[\w ]+\s+{name}\s*=\s*([^;]+);", src)
    assert m, name
    return m.group(1)


def test_lane_bound_of_the_header():
    """The int32 lane bound stated in csrc/spgg_reputation.h, recomputed from its constants: a lane
    adds at most kMaxLaneDots dots of magnitude <= 4 * 128^2, the LDS instances stay below that at
    their largest side, and the reported side is the largest at which the global instance does."""
    src = open(KERNEL_HEADER).read()
    assert _constant(src, "kCellsPerDword") == "4" and _constant(src, "kThreads") == "1024"
    assert _constant(src, "kDotMax").replace("ll", "") == "4 * 128 * 128"
    assert _constant(src, "kFullDwords") == "163840 / 4" and _constant(src, "kSmallDwords") == "65536 / 4"
    dot_max = 4 * 128 * 128
    assert K.DOT_MAX == dot_max == 4 * (-128) * (-128)   # the largest product is (-128)^2
    max_lane_dots = (2 ** 31 - 1) // dot_max
    assert max_lane_dots == 32767
    assert max_lane_dots * dot_max < 2 ** 31 <= (max_lane_dots + 1) * dot_max

    def lattice(L):
        return L * K.row_dwords(L)

    def lane_dots_lds(L):      # one wave of 64 lanes sums a pair over all L * W dwords
        W = K.row_dwords(L)
        cols = -(-lattice(L) // 64)                                         # lane l: dwords l, l + 64, ..
        rows = -(-L // (64 // W)) if W <= 64 else L * -(-W // 64)           # one dword index, every (64 // W)-th row
        return max(rows, cols)

    def lane_dots_global(L):   # wave v of 16 takes the rows v, v + 16, .., lane l the dwords l, l + 64, ..
        return -(-L // K.WAVES) * -(-K.row_dwords(L) // 64)

    lds_side = max(L for L in range(1, 1000) if lattice(L) <= K.FULL_DWORDS)
    assert lds_side == 404 and "404" in src
    assert max(lane_dots_lds(L) for L in range(1, lds_side + 1)) == lane_dots_lds(lds_side) == 808 <= max_lane_dots
    assert max(L for L in range(1, 1000) if lattice(L) <= K.SMALL_DWORDS) == 256
    side = lds_side
    while lane_dots_global(side + 1) <= max_lane_dots:
        side += 1
    assert side == 11520 and re.search(r"static_assert\(kMaxSide == 11520", src)
    assert side >= 1000 and side * side < 2 ** 31
    assert "11520" in open(HEADER).read()
    # the issue's figure for a one-pair-per-wave split: ceil(n / 256) dots per lane up to side 2896
    assert -(-2896 * 2896 // 256) <= max_lane_dots < -(-2897 * 2897 // 256)


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(spgg_\w+)\s*\(", src, flags=re.M))


def test_abi_v19():
    """Header = binding = exports, version 19, the three new entry points among them."""
    new = {"spgg_reputation_hist", "spgg_reputation_pairs", "spgg_reputation_max_side"}
    assert new <= _declared(HEADER) == set(_lib.EXPORTED)
    assert int(re.search(r"#define SPGG_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == _lib.ABI_VERSION == 19
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    assert lib.spgg_abi_version() == 19
    assert all(hasattr(lib, name) for name in _lib.EXPORTED)
    # null arguments fail with SPGG_E_ARG before any device call
    side = ctypes.c_int32(-5)
    assert lib.spgg_reputation_max_side(None, ctypes.byref(side)) == _lib.E_ARG and side.value == -5
    out = (ctypes.c_int64 * 4)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert lib.spgg_reputation_pairs(None, 1, 0, p, 4, None) == _lib.E_ARG
    assert lib.spgg_reputation_hist(None, 1, 1, p, p, 4, None) == _lib.E_ARG
    assert list(out) == [0, 0, 0, 0]


def test_kernel_resources(tmp_path):
    """Pair sums: two LDS instances and one that declares no lattice; the small one declares 64 KiB
    (two workgroups share a CU), the full one what a workgroup may declare.  No scratch, no spills."""
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
        blocks += [b for b in notes.split("- .agpr_count:")[1:] if "spgg_reputation_" in b]

    def field(b, k):
        return int(re.search(rf"\.{k}:\s+(\d+)", b).group(1))

    def named(part):
        return [b for b in blocks if part in b]

    assert len(named("pairs_lds_kernel")) == 2 and len(named("pairs_global_kernel")) == 1
    assert len(named("hist_kernel")) == 2 and len(blocks) == 6   # + the launch that zeroes the rows
    lds = sorted(field(b, "group_segment_fixed_size") for b in named("pairs_lds_kernel"))
    assert lds == [4 * K.SMALL_DWORDS, 4 * K.FULL_DWORDS] and lds[1] <= 163840
    assert 4 * 404 * K.row_dwords(404) <= lds[1] < 4 * 405 * K.row_dwords(405)
    assert field(named("pairs_global_kernel")[0], "group_segment_fixed_size") <= 1024
    for b in named("hist_kernel"):
        assert field(b, "group_segment_fixed_size") <= 16384   # several workgroups per CU
    for b in blocks:
        assert field(b, "private_segment_fixed_size") == 0
        assert field(b, "vgpr_spill_count") == 0 and field(b, "sgpr_spill_count") == 0
    for b in named("pairs_"):
        assert field(b, "max_flat_workgroup_size") == 1024


def test_write_datasets_takes_the_reputation_record(tmp_path, monkeypatch):
    monkeypatch.setenv("SPGG_H5_SINK", "npz")
    c = Case("m1_rep_L16")
    snaps = {int(k[11:]): (c.datasets[k], c.datasets["Sn_snapshot_" + k[11:]])
             for k in c.datasets if k.startswith("R_snapshot_")}

    def write(name, **kw):
        fn = str(tmp_path / name)
        spgg.write_datasets(fn, c.datasets, snaps, c.Sn, c.R, c.kwargs.get("R_min", -10), c.kwargs.get("R_max", 10),
                            spgg.track_positions(c.kwargs["L"]), **kw)
        return read_datasets(fn)

    hist = dict(reputation_history_iters=np.array([1, 6]),
                reputation_hist_history=np.arange(2 * 2 * 20, dtype=np.int32).reshape(2, 2, 20),
                reputation_bin_edges=np.linspace(-10, 10, 21))
    pairs = dict(reputation_sum_history=np.array([3, -4]), reputation_pair_rows_history=np.arange(10).reshape(2, 5),
                 reputation_pair_cols_history=np.arange(10, 20).reshape(2, 5), reputation_unit=np.float64(0.5))
    assert set(spgg.REPUTATION_DATASETS) == set(hist) | set(pairs)
    base = write("b.npz")
    assert sorted(base) == sorted(c.datasets)
    got = write("a.npz", records=dict(reputation=hist))
    assert set(got) - set(base) == set(hist)
    got = write("c.npz", records=dict(reputation=dict(hist, **pairs)))
    assert set(got) - set(base) == set(hist) | set(pairs)
    for k, v in dict(hist, **pairs).items():
        want = np.float64 if k in ("reputation_bin_edges", "reputation_unit") else np.int64
        assert got[k].dtype == want and np.array_equal(got[k], v), k
    assert (spgg.SPGG.reputation_history_every, spgg.SPGG.reputation_history_bins,
            spgg.SPGG.reputation_max_distance) == (0, 20, None)


def test_sweep_pops_the_overrides(tmp_path, monkeypatch):
    """The three options are class attributes of the drop-in: run_one_experiment and run_batch take
    them among the model overrides and keep them from the constructor and from RUNNER_MODEL's keys."""
    from spgg_amd import engine as E
    from spgg_amd import sweep as SW
    monkeypatch.chdir(tmp_path)
    params = (3.0, 1.0, False, 0.8, 1.0, 1.0, "reputation", "qlearning")
    seen = {}

    class FakeSPGG:
        rep_avg_history = []

        def __init__(self, **kw):
            assert not {k for k in kw if k.startswith("reputation_")}, kw
            seen["ctor"] = kw

        def run(self, filename):
            seen["attrs"] = (self.reputation_history_every, self.reputation_history_bins, self.reputation_max_distance)
            return 0.5, 0.5, None

    monkeypatch.setattr(spgg, "SPGG", FakeSPGG)
    SW.run_one_experiment(params, L=8, iterations=3, reputation_history_every=5, reputation_history_bins=7,
                          reputation_max_distance=4)
    assert seen["attrs"] == (5, 7, 4) and seen["ctor"]["L"] == 8
    SW.run_one_experiment(params, L=8, iterations=3)
    assert seen["attrs"] == (0, 20, None)

    class FakeEngine:
        def __init__(self, L, iterations, replicas, **kw):
            self.L, self.R = L, len(replicas)
            self.snapshots = [dict() for _ in replicas]
            self.png_frames = [dict() for _ in replicas]

        def run(self, **kw):
            seen["run"] = kw

        def histories(self):
            return [dict() for _ in range(self.R)]

        def reputation_histories(self):
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
                 reputation_history_every=2, reputation_history_bins=9, reputation_max_distance=3)
    run = seen["run"]
    assert (run["reputation_every"], run["reputation_bins"], run["reputation_max_d"]) == (2, 9, 3)
    assert run["clusters_every"] == 0 and run["correlations_every"] == 0 and seen.pop("asked")
    assert [w["records"]["reputation"] for w in written] == [dict(marker=0), dict(marker=1)]
    written.clear()
    SW.run_batch([params], seeds=[1], save_png=False, verbose=False, L=8, iterations=3)
    run = seen["run"]
    assert (run["reputation_every"], run["reputation_bins"], run["reputation_max_d"]) == (0, 20, None)
    assert "asked" not in seen and written[0]["records"]["reputation"] is None
