"""The pair maps on the CPU (no device): the host model (spgg_amd.pairmap: np.roll, the definition itself),
the NumPy model of the device's packing and windowing (tests/_pairmap.py) held to it, the identities that
tie the map to spgg_correlations and to the history record, the derived quantities, the work formula
against the library's own, the option tables, the record's schedule and refusals on a stub engine, and the
header against the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import spgg_oracle as O
from spgg_amd import _lib, pairmap as PM, records
from tests import _pairmap as K

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spgg_abi.h")
SIDES = (1, 2, 3, 5, 13, 31, 32, 33, 37, 64, 70, 100)


def _fields(L, name, seed=0):
    S, prev = K.patterns(L, seed)[name]
    return PM.host_fields(K.byte_plane(S, prev, 7 * L + seed), 2)


# ---- the kernel's scheme against the definition ---------------------------------------------------------------------
@pytest.mark.parametrize("L", SIDES)
def test_kernel_model_equals_roll(L):
    f = _fields(L, "random")
    for D in sorted({L // 2, K.smaller(L)}):
        for a, b in K.PAIRS:
            want = PM.host_pair_map(f[a], f[b], D)
            got = K.model_pair_map(f[a], f[b], D)
            assert want.shape == PM.map_shape(D) == got.shape and want.dtype == np.int64
            assert np.array_equal(got, want), (L, D, a, b, np.argwhere(got != want)[:6].tolist())
            assert np.array_equal(PM.host_pair_map_fft(f[a], f[b], D), want), (L, D, a, b)


def test_host_fields_read_bits_0_and_3_alone():
    L = 13
    S, prev = K.patterns(L)["random"]
    clean = (S | prev << 3).astype(np.uint8)
    for seed in (1, 2):
        dirty = K.byte_plane(S, prev, seed)
        assert np.any(dirty & ~np.uint8(K.KEEP)) and np.array_equal(dirty & K.KEEP, clean)
        for t in (1, 2, 9):
            got, want = PM.host_fields(dirty, t), PM.host_fields(clean, t)
            assert all(np.array_equal(got[k], want[k]) and got[k].dtype == bool for k in PM.FIELDS)
    f1, f2 = PM.host_fields(clean, 1), PM.host_fields(clean, 2)
    assert not f1["flip"].any() and np.array_equal(f2["flip"], S != prev) and f2["flip"].any()
    assert np.array_equal(f1["coop"], S == 0) and np.array_equal(f2["coop"], S == 0)
    with pytest.raises(ValueError):
        PM.host_fields(clean, 0)
    with pytest.raises(ValueError):
        PM.host_pair_map(f2["coop"], f2["coop"], L // 2 + 1)


@pytest.mark.parametrize("L", (1, 2, 3, 4, 5, 13, 32, 37, 100))
def test_axis_identities_with_the_pair_counts(L):
    """map_CC[0][D + d] = map_CC[0][D - d] = rows[d] and map_CC[d][D] = cols[d] of spgg_correlations' host model; at
    even L the columns dx = -D and dx = +D of D = L / 2 are the same displacement."""
    D = L // 2
    for name in ("random", "checkerboard", "one_cell"):
        S, _prev = K.patterns(L)[name]
        c = S == 0
        m = PM.host_pair_map(c, c, D)
        pc = records.host_pair_counts(S, D)
        assert np.array_equal(m[0, D:], pc[0]) and np.array_equal(m[0, D::-1], pc[0]), (L, name)
        assert np.array_equal(m[:, D], pc[1]), (L, name)
        if L % 2 == 0:
            assert np.array_equal(m[:, 0], m[:, 2 * D]), (L, name)
        assert m.max() <= L * L and m[0, D] == np.count_nonzero(c)


def test_flip_count_is_the_history_records_switches():
    """map_FF[0][D] of S_t is SW_CD + SW_DC of iteration t - 1, on an oracle run."""
    L, T = 10, 12
    p = O.Params(L=L, iterations=T)
    states = {}
    ds, _fin = O.run(p, np.random.RandomState(3), collect_snapshots=False,
                     on_step=lambda i, S, R, Q, d: states.__setitem__(i + 1, np.array(S, dtype=np.uint8)))
    seen = 0
    for t in range(3, T + 1):
        byte = states[t] | (states[t - 1] << 3)
        f = PM.host_fields(byte, t)
        m = PM.host_pair_map(f["flip"], f["flip"], 2)
        assert m[0, 2] == ds["switch_C_to_D"][t - 2] + ds["switch_D_to_C"][t - 2], t
        seen += int(m[0, 2])
    assert seen > 0


@pytest.mark.parametrize("L", (2, 3, 5, 8, 13))
def test_the_other_half_plane_is_the_swapped_map(L):
    f = _fields(L, "random")
    D = L // 2
    ab, ba = PM.host_pair_map(f["coop"], f["flip"], D), PM.host_pair_map(f["flip"], f["coop"], D)
    for dy in range(D + 1):
        for dx in range(-D, D + 1):
            direct = np.count_nonzero(f["coop"] & np.roll(f["flip"], (dy, dx), axis=(0, 1)))      # the displacement (-dx, -dy)
            assert direct == ba[dy, dx + D], (L, dy, dx)
    full = PM.full_plane(ab, ba)
    assert full.shape == (2 * D + 1, 2 * D + 1)
    for dy in range(-D, D + 1):
        for dx in range(-D, D + 1):
            assert full[dy + D, dx + D] == np.count_nonzero(f["coop"] & np.roll(f["flip"], (-dy, -dx), axis=(0, 1))), (L, dy, dx)
    cc = PM.host_pair_map(f["coop"], f["coop"], D)
    auto = PM.full_plane(cc)
    assert np.array_equal(auto, auto[::-1, ::-1])
    with pytest.raises(ValueError):
        PM.full_plane(ab, ba[:-1])


def test_orientation():
    """One cell of A against an asymmetric B: the map is B seen from that cell.  A swapped sign or axis moves the
    figure; every symmetric pattern hides both."""
    L, D = 11, 5
    B = K.l_figure(L)
    assert not np.array_equal(B, B.T) and not np.array_equal(B, B[::-1]) and not np.array_equal(B, B[:, ::-1])
    y0, x0 = L // 4, L // 3           # the figure's corner: it lies at dy = 0 .. 2, dx = 0 .. 1 from there
    A = np.zeros((L, L), dtype=bool)
    A[y0, x0] = True
    want = np.zeros(PM.map_shape(D), dtype=np.int64)
    for dy, dx in ((0, 0), (1, 0), (2, 0), (2, 1)):
        want[dy, dx + D] = 1
    for fn in (PM.host_pair_map, K.model_pair_map, PM.host_pair_map_fft):
        assert np.array_equal(fn(A, B, D), want), fn.__name__
    swapped = PM.host_pair_map(B, A, D)          # the figure seen from its cells: the one cell lies at (-dx, -dy)
    assert swapped[0, D] == 1 and swapped.sum() == 1 + 0      # only (0, 0) has dy >= 0 among the four, mirrored
    assert np.array_equal(PM.full_plane(want, swapped)[D:], want)
    assert PM.full_plane(want, swapped)[:D].sum() == 0 and PM.full_plane(swapped, want)[:D].sum() == 3


# ---- derived quantities ----------------------------------------------------------------------------------------------
def test_radial_function():
    D = 6
    d = np.arange(-D, D + 1)
    r = np.rint(np.hypot(d[:, None], d[None, :])).astype(int)
    for L in (13, 20):
        n = L * L
        full_c = np.ones((L, L), dtype=bool)
        G, count = PM.radial_function(PM.host_pair_map(full_c, full_c, D), n, 1.0, 1.0)
        assert G.shape == count.shape == (D + 1,) and np.array_equal(G, np.zeros(D + 1))      # a constant field
        assert count.tolist() == [int(np.sum(r == k)) for k in range(D + 1)] and count[0] == 1 and count[1] == 8
        f = _fields(L, "random")
        rho = f["coop"].mean()
        m = PM.host_pair_map(f["coop"], f["coop"], D)
        G, count2 = PM.radial_function(m, n, rho, rho)
        assert np.array_equal(count2, count)
        full = PM.full_plane(m) / n - rho * rho
        for k in range(D + 1):
            assert abs(G[k] - full[r == k].mean()) <= 1e-15, (L, k)
        assert G[0] == rho - rho * rho or abs(G[0] - (rho - rho * rho)) < 1e-15
        assert np.isfinite(records.correlation_length(G)) or records.correlation_length(G) == float("inf")
        mf = PM.host_pair_map(f["coop"], f["flip"], D)
        Gx, _ = PM.radial_function(mf, n, rho, f["flip"].mean(), PM.host_pair_map(f["flip"], f["coop"], D))
        fullx = PM.full_plane(mf, PM.host_pair_map(f["flip"], f["coop"], D)) / n - rho * f["flip"].mean()
        assert abs(Gx[3] - fullx[r == 3].mean()) <= 1e-15


@pytest.mark.parametrize("L", (1, 2, 5, 8, 13, 32))
def test_structure_factor_is_wiener_khinchin(L):
    f = _fields(L, "random")
    A = f["coop"].astype(np.float64)
    m = PM.host_pair_map(f["coop"], f["coop"])
    Sk = PM.structure_factor(m, L)
    want = np.abs(np.fft.fft2(A)) ** 2 / (L * L)
    assert Sk.shape == (L, L)
    assert np.max(np.abs(Sk - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), L
    B = f["flip"].astype(np.float64)
    cross = PM.structure_factor(PM.host_pair_map(f["coop"], f["flip"]), L, PM.host_pair_map(f["flip"], f["coop"]))
    wantx = np.conj(np.fft.fft2(A)) * np.fft.fft2(B) / (L * L)
    assert np.max(np.abs(cross - wantx)) <= 1e-12 * max(1.0, np.max(np.abs(wantx))), L
    if L >= 4:
        with pytest.raises(ValueError, match="L // 2"):
            PM.structure_factor(PM.host_pair_map(f["coop"], f["coop"], L // 2 - 1), L)


# ---- work and cap ----------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 0), (2, 3, 1), (13, 2, 6), (32, 1, 16), (33, 7, 15), (200, 105, 32), (200, 105, 100), (200, 8, 100), (1000, 1, 500),
          (1000, 1, 2), (32768, 1, 16384), (32768, 40000, 16384)]


def test_work_formula():
    assert PM.work(200, 105, 32) == 105 * 33 * 3 * 200 * 7 == 14_553_000
    assert PM.work(1000, 1, 500) == 501 * 32 * 1000 * 32 == 513_024_000
    assert PM.work(1000, 1, 500) <= PM.WORK_CAP and PM.work(200, 105, 100) <= PM.WORK_CAP      # the shapes of the issue
    assert PM.work(32768, 1, 16384) > PM.WORK_CAP
    assert PM.work(32768, 40000, 16384) == 2 ** 63 - 1                                          # saturates
    assert K.plane_words(1000, 500) * 4 == 384_000 and K.plane_words(200, 32) == 200 * (7 + 10)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    w, cap = ctypes.c_int64(), ctypes.c_int64()
    for L, n_rep, D in SHAPES:
        assert lib.spgg_pair_map_work(L, n_rep, D, ctypes.byref(w), ctypes.byref(cap)) == _lib.OK
        assert w.value == PM.work(L, n_rep, D) and cap.value == PM.WORK_CAP == _lib.PAIR_MAP_WORK_CAP, (L, n_rep, D)
    for bad in ((0, 1, 0), (8, 0, 1), (8, 1, -1), (8, 1, 5)):
        assert lib.spgg_pair_map_work(*bad, ctypes.byref(w), ctypes.byref(cap)) == _lib.E_ARG, bad
    assert lib.spgg_pair_map_work(8, 1, 1, None, ctypes.byref(cap)) == _lib.E_ARG


# ---- header, binding, option tables ------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree():
    text = open(HEADER).read()
    assert int(re.search(r"#define SPGG_ABI_VERSION (\d+)", text).group(1)) == 19 == _lib.ABI_VERSION
    assert int(re.search(r"#define SPGG_FIELD_COOP (\d+)", text).group(1)) == PM.FIELDS["coop"] == _lib.FIELD_COOP == 0
    assert int(re.search(r"#define SPGG_FIELD_FLIP (\d+)", text).group(1)) == PM.FIELDS["flip"] == _lib.FIELD_FLIP == 1
    assert int(re.search(r"#define SPGG_PAIR_MAP_WORK_CAP (\d+)ll", text).group(1)) == _lib.PAIR_MAP_WORK_CAP == PM.WORK_CAP
    assert list(PM.FIELDS) == ["coop", "flip"] and PM.map_shape(0) == (1, 1) and PM.map_shape(32) == (33, 65)
    names = {"spgg_pair_map_work": ["L", "n_rep", "max_d", "work", "cap"],
             "spgg_pair_map_workspace": ["ctx", "max_d", "words_per_rep"],
             "spgg_pair_map": ["ctx", "t", "field_a", "field_b", "max_d", "work", "out", "out_stride", "hip_stream"]}
    for fn, want in names.items():
        proto = re.search(rf"int {fn}\(([^)]*)\);", text).group(1)
        args = [a.strip().split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
        assert args == want and fn in _lib.EXPORTED, fn
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    for fn, want in names.items():
        f = getattr(lib, fn)
        assert f.restype is ctypes.c_int and len(f.argtypes) == len(want), fn
    assert lib.spgg_pair_map(None, 1, 0, 0, 0, None, None, 1, None) == _lib.E_ARG          # a null context
    assert lib.spgg_pair_map_workspace(None, 0, None) == _lib.E_ARG


def test_option_tables():
    from spgg_amd import spgg, sweep
    """The pair-map options through the one entry point (the table itself: tests/test_records_cpu.py)."""
    mine = ["pair_map_history_every", "pair_map_max_distance", "pair_map_fields"]

    def values(v):
        return {k: x for k, x in spgg.record_options(v)[0].items() if k.startswith("pair_map")}

    assert [o[0] for o in PM.PairMap.options] == mine
    assert (spgg.SPGG.pair_map_history_every, spgg.SPGG.pair_map_max_distance, spgg.SPGG.pair_map_fields) == (0, None, (("coop", "coop"),))
    kw = dict(L=8, pair_map_history_every="3", pair_map_max_distance=2, pair_map_fields=[["coop", "coop"], ["flip", "coop"]], epsilon=0.2)
    got = {k: v for k, v in sweep.pop_record_options(kw).items() if k in mine}
    assert got == dict(pair_map_history_every=3, pair_map_max_distance=2, pair_map_fields=(("coop", "coop"), ("flip", "coop")))
    assert kw == dict(L=8, epsilon=0.2)
    assert {k: v for k, v in sweep.pop_record_options({}).items() if k in mine} == {o[0]: o[2] for o in PM.PairMap.options}
    assert values(got) == dict(pair_map_every=3, pair_map_max_d=2, pair_map_fields=(("coop", "coop"), ("flip", "coop")))
    assert values({}) == dict(pair_map_every=0, pair_map_max_d=None, pair_map_fields=(("coop", "coop"),))
    with pytest.raises(ValueError, match="pair_map_max_distance needs pair_map_history_every > 0"):
        values(dict(pair_map_max_distance=2))
    for bad in (dict(pair_map_history_every=2, pair_map_fields=(("coop", "state"),)),
                dict(pair_map_history_every=2, pair_map_fields=(("coop", "coop"), ("coop", "coop"))),
                dict(pair_map_history_every=2, pair_map_fields=())):
        with pytest.raises(ValueError, match="pair_map_fields"):
            values(bad)
    assert records.KINDS["pair_map"] is PM.PairMap and issubclass(PM.PairMap, records.Record)
    assert PM.dataset_name("coop", "flip") == "pair_map_coop_flip_history"


class _Eng:
    """What PairMap.validate reads of an engine."""
    def __init__(self, L=18, groups=((0, 3),)):
        self.L, self.groups = L, [dict(r0=a, r1=b) for a, b in groups]


def test_record_key_schedule_and_refusals():
    V = PM.PairMap.validate
    cc = (("coop", "coop"),)
    assert V(_Eng(), 0, None, cc) == (0, None, ()) == V(_Eng(), 0, 99, "whatever")          # unarmed: nothing is looked at
    assert V(_Eng(), 3, None, cc) == (3, 9, cc) and V(_Eng(200), "3", None, cc) == (3, 32, cc)      # min(L // 2, 32)
    assert V(_Eng(200), 5, 100, [["coop", "flip"], ("flip", "flip")]) == (5, 100, (("coop", "flip"), ("flip", "flip")))
    for every, D, fields in ((-1, None, cc), (2, -1, cc), (2, 10, cc), (2, 3, (("coop", "rep"),)), (2, 3, (("coop", "coop"),) * 2),
                             (2, 3, ()), (2, 3, "cc"), (2, 3, (("coop",),))):
        with pytest.raises(ValueError):
            V(_Eng(), every, D, fields)
    # the cap: through pairmap.work, the largest replica group's call
    big = _Eng(32768, ((0, 1),))
    assert PM.work(32768, 1, 16384) > PM.WORK_CAP
    with pytest.raises(ValueError, match="cap"):
        V(big, 1, 16384, cc)
    assert V(big, 1, None, cc) == (1, 32, cc) and PM.work(32768, 1, 32) <= PM.WORK_CAP
    fit = PM.WORK_CAP // PM.work(1000, 1, 500)          # replicas of cfg5's lattice at D = 500 that one call may hold
    assert fit >= 1 and PM.work(1000, fit, 500) <= PM.WORK_CAP < PM.work(1000, fit + 1, 500)
    assert V(_Eng(1000, ((0, fit), (fit, 2 * fit))), 1, 500, cc) == (1, 500, cc)
    with pytest.raises(ValueError, match="cap"):
        V(_Eng(1000, ((0, fit), (fit, 2 * fit + 1))), 1, 500, cc)
    # the schedule and the row layout are the Record's
    rec = PM.PairMap(3, 5, 20, (3, 2, (("coop", "coop"), ("coop", "flip"))))
    assert rec.rows == 6 and [t for t in range(1, 21) if t >= 5 and rec.due(t)] == [5, 8, 11, 14, 17, 20]
    assert rec.next_due(5) == 8 and rec.next_due(6) == 8 and rec.row(11) == 2

    class _E:
        R = 1
    its = rec.iters(12)
    rows = [np.arange(len(its) * 15).reshape(len(its), 15), np.arange(len(its) * 15).reshape(len(its), 15) + 1]
    d = rec.datasets(_E(), 0, its, *rows)
    assert list(d) == ["pair_map_history_iters", "pair_map_max_distance", "pair_map_coop_coop_history", "pair_map_coop_flip_history"]
    assert d["pair_map_max_distance"] == 2 and d["pair_map_coop_flip_history"].shape == (3, 3, 5)
    assert np.array_equal(d["pair_map_coop_coop_history"][1], np.arange(15, 30).reshape(3, 5))


def test_datasets_reach_the_sinks(tmp_path, monkeypatch):
    """write_datasets puts the pair-map datasets after the payoff datasets -- the iterations, one map history per
    pair, the distance -- through every available sink; without the record the file holds the set it held before."""
    from spgg_amd import h5io, spgg
    rs = np.random.RandomState(4)
    L, m, D = 4, 2, 1
    hist = {name: np.zeros(0) for name in spgg.HISTORY_DATASETS}
    hist.update({f"group_comp_d{d}_history": np.zeros(0) for d in range(6)})
    hist.update({f"{g}_q_{s}_{a}_history": np.zeros(0) for g in ("cooperators", "defectors", "avg") for s in ("s0", "s1") for a in "cd"})
    ph = {"pair_map_history_iters": np.arange(1, m + 1), "pair_map_max_distance": np.int64(D),
          "pair_map_coop_coop_history": rs.randint(0, 9, (m,) + PM.map_shape(D)),
          "pair_map_flip_coop_history": rs.randint(0, 9, (m,) + PM.map_shape(D))}
    order = ["pair_map_history_iters", "pair_map_coop_coop_history", "pair_map_flip_coop_history", "pair_map_max_distance"]
    S, Rn = rs.randint(0, 2, (L, L)), np.zeros((L, L))
    sinks = ("npz",) + (("native",) if h5io.h5native.available() else ())
    try:
        import h5py  # noqa: F401
        sinks += ("h5py",)
    except ImportError:
        pass
    for sink in sinks:
        monkeypatch.setenv("SPGG_H5_SINK", sink)
        fn = str(tmp_path / f"{sink}.h5")
        spgg.write_datasets(fn, hist, {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64))
        plain = list(h5io.read_datasets(fn))
        assert not set(ph) & set(plain)
        spgg.write_datasets(fn, hist, {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64), records=dict(pair_map=ph))
        got = h5io.read_datasets(fn)
        for name, want in ph.items():
            assert got[name].dtype == np.int64, (sink, name)
            if np.ndim(want) == 0:          # (a sink may hold a scalar as one element)
                assert got[name].size == 1 and got[name].ravel()[0] == want, (sink, name)
            else:
                assert got[name].shape == want.shape and np.array_equal(got[name], want), (sink, name)
        assert set(got) == set(plain) | set(ph), sink
        if sink == "npz":
            assert list(got) == plain + order, list(got)[-6:]
