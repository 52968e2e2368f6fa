"""The learned policy record on the CPU: the NumPy host model against a literal per-agent loop, its
invariants, the edge rule against np.histogram, the ABI's three statements of spgg_policy, the option
tables and every refusal that needs no device, and the built kernels' register budget.  No GPU."""
import os
import re

import numpy as np
import pytest

from spgg_amd import _lib, policy as PL
from tests import test_kernel_resources_cpu as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgg_abi.h")


def _literal(Q, S, state, bins, edges):
    """The record as spgg_abi.h words it, one agent at a time."""
    L = S.shape[0]
    row = [0] * PL.policy_width(bins)
    plane = np.zeros((L, L), dtype=np.uint8)

    def cls(y, x):
        g = [0 if Q[y, x, s, 0] >= Q[y, x, s, 1] else 1 for s in (0, 1)]
        return g[0] + 2 * g[1]

    for y in range(L):
        for x in range(L):
            c, sg, z = cls(y, x), int(S[y, x]) & 1, int(state[y, x]) & 1
            row[c * 4 + sg * 2 + z] += 1
            plane[y, x] = c | sg << 2 | z << 3
            for other in (cls(y, (x + 1) % L), cls((y + 1) % L, x)):
                row[16 + c if other == c else 20] += 1
            for s in (0, 1):
                gap = Q[y, x, s, 0] - Q[y, x, s, 1]
                if gap < edges[0]:
                    slot = 0
                elif gap > edges[bins]:
                    slot = bins + 1
                else:
                    slot = 1 + next(i for i in range(bins) if edges[i] <= gap < edges[i + 1] or (i == bins - 1 and gap == edges[bins]))
                row[21 + (sg * 2 + s) * (bins + 2) + slot] += 1
    return np.array(row, dtype=np.int64), plane


def _case(L, seed, ties=True):
    rs = np.random.RandomState(seed)
    Q = rs.uniform(-1, 1, (L, L, 2, 2))
    if ties:
        Q[rs.rand(L, L) < 0.3, 0, 1] = 0.0
        Q[rs.rand(L, L) < 0.3, 0, 0] = 0.0        # equal entries: the tie goes to action 0
    return Q, rs.randint(0, 2, (L, L)), rs.randint(0, 2, (L, L))


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("bins,gap_range", [(1, 0.5), (4, 0.25), (7, (-0.1, 1.5))])
def test_host_model_against_a_literal_loop(L, bins, gap_range):
    edges = PL.policy_bin_edges(gap_range, bins)
    for seed in range(6):
        Q, S, z = _case(L, 10 * L + seed)
        row, plane = PL.host_policy_record(Q, S, z, bins, edges)
        want, want_plane = _literal(Q, S, z, bins, edges)
        assert row.dtype == np.int64 and plane.dtype == np.uint8
        assert np.array_equal(row, want), (L, seed, row.tolist(), want.tolist())
        assert np.array_equal(plane, want_plane)


def test_aliased_bonds_of_tiny_lattices():
    Q, S, z = _case(1, 3)
    row, _ = PL.host_policy_record(Q, S, z, 2, PL.policy_bin_edges(1.0, 2))
    assert row[16:21].sum() == 2 and row[20] == 0           # one agent: both bonds join it to itself
    Q = np.zeros((2, 2, 2, 2))
    Q[0, 0, 0] = (0.0, 1.0)                                  # one agent of class 1 among three of class 0
    row, _ = PL.host_policy_record(Q, np.zeros((2, 2)), np.zeros((2, 2)), 2, PL.policy_bin_edges(1.0, 2))
    assert row[16:21].tolist() == [4, 0, 0, 0, 4]           # each of its two neighbours is met twice


@pytest.mark.parametrize("L", [2, 5, 9])
def test_invariants(L):
    bins = 6
    edges = PL.policy_bin_edges(0.4, bins)
    for seed in range(4):
        Q, S, z = _case(L, 100 + seed)
        row, plane = PL.host_policy_record(Q, S, z, bins, edges)
        counts, bonds, hist = PL.split_row(row, bins)
        n = L * L
        assert counts.sum() == n and bonds.sum() == 2 * n
        for sg in (0, 1):
            assert counts[:, sg].sum() == np.count_nonzero(S == sg)
            assert hist[sg].sum(axis=1).tolist() == [np.count_nonzero(S == sg)] * 2       # nothing is dropped
        assert np.array_equal(plane & 3, PL.policy_classes(Q)) and np.array_equal(plane >> 2 & 1, S)
        assert np.array_equal(plane >> 3, z)
        key = (plane & 3) * 4 + (plane >> 2 & 1) * 2 + (plane >> 3)
        assert np.array_equal(np.bincount(key.ravel(), minlength=16), counts.ravel())


def test_edge_rule_against_np_histogram():
    bins = 5
    edges = PL.policy_bin_edges((-0.5, 0.75), bins)
    below, above = np.nextafter(edges[0], -1), np.nextafter(edges[-1], 2)
    gaps = np.concatenate([edges, [below, above, -3.0, 3.0], np.nextafter(edges, -1), np.nextafter(edges, 2)])
    got = PL.policy_gap_hist(gaps, edges)
    assert np.array_equal(got[1:-1], np.histogram(gaps, bins=bins, range=(-0.5, 0.75))[0])
    assert got[0] == np.count_nonzero(gaps < edges[0]) == 3 and got[-1] == np.count_nonzero(gaps > edges[-1]) == 3
    assert got.sum() == gaps.size
    only = PL.policy_gap_hist([edges[-1]], edges)            # x == edges[bins]: the last bin, not the slot above
    assert only[bins] == 1 and only.sum() == 1
    assert PL.policy_gap_hist([edges[0]], edges)[1] == 1
    # through the record: an agent whose gap is the last edge
    Q = np.zeros((1, 1, 2, 2))
    Q[0, 0, 0] = (edges[-1], 0.0)
    row, _ = PL.host_policy_record(Q, np.zeros((1, 1)), np.zeros((1, 1)), bins, edges)
    assert PL.split_row(row, bins)[2][0, 0, bins] == 1
    assert np.array_equal(PL.policy_bin_edges(2.0, 32), np.histogram_bin_edges(np.empty(0), 32, (-2.0, 2.0)))


def test_header_binding_and_exports_agree():
    text = open(HEADER).read()
    assert int(re.search(r"#define SPGG_ABI_VERSION (\d+)", text).group(1)) == 19 == _lib.ABI_VERSION
    assert int(re.search(r"#define SPGG_POLICY_COUNTS (\d+)", text).group(1)) == _lib.POLICY_COUNTS == PL.POLICY_COUNTS == 21
    proto = re.search(r"int spgg_policy\(([^)]*)\);", text).group(1)
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "t", "bins", "edges", "plane", "out", "out_stride", "hip_stream"]
    assert "spgg_policy" in _lib.EXPORTED
    assert PL.policy_width(32) == 21 + 4 * 34 and PL.policy_width(1) == 33
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    assert lib.spgg_abi_version() == 19
    fn = lib.spgg_policy
    assert fn.restype is __import__("ctypes").c_int and len(fn.argtypes) == len(args)
    assert fn(None, 1, 4, None, None, None, 64, None) == _lib.E_ARG          # a null context


def test_option_tables():
    from spgg_amd import spgg, sweep
    """The policy options through the one entry point (the table itself: tests/test_records_cpu.py)."""
    mine = ["policy_history_every", "policy_history_bins", "policy_history_gap_range", "policy_map_final"]

    def values(v):
        run_kw, extras = spgg.record_options(v)
        return {k: x for k, x in run_kw.items() if k.startswith("policy")}, extras["policy_map_final"]

    assert [o[0] for o in PL.Policy.options] == mine
    assert (spgg.SPGG.policy_history_every, spgg.SPGG.policy_history_bins, spgg.SPGG.policy_history_gap_range,
            spgg.SPGG.policy_map_final) == (0, 32, 2.0, False)
    kw = dict(L=8, policy_history_every="3", policy_history_bins=16, policy_map_final=1, epsilon=0.2)
    got = {k: v for k, v in sweep.pop_record_options(kw).items() if k in mine}
    assert got == dict(policy_history_every=3, policy_history_bins=16, policy_history_gap_range=2.0, policy_map_final=True)
    assert kw == dict(L=8, epsilon=0.2)
    assert {k: v for k, v in sweep.pop_record_options({}).items() if k in mine} == {o[0]: o[2] for o in PL.Policy.options}
    run_kw, final = values(got)
    assert run_kw == dict(policy_every=3, policy_bins=16, policy_gap_range=2.0) and final is True
    assert values({}) == (dict(policy_every=0, policy_bins=32, policy_gap_range=2.0), False)
    with pytest.raises(ValueError, match="policy_map_final needs policy_history_every > 0"):
        values(dict(policy_map_final=True))
    from spgg_amd import records
    assert records.KINDS["policy"] is PL.Policy and issubclass(PL.Policy, records.Record)
    assert PL.POLICY_DATASETS == ("policy_history_iters", "policy_count_history", "policy_bond_history",
                                  "policy_gap_hist_history", "policy_gap_bin_edges")


class _Eng:
    persistent = False


def test_every_value_error():
    for bins in (0, 257, -1):
        with pytest.raises(ValueError):
            PL.policy_bin_edges(1.0, bins)
        with pytest.raises(ValueError):
            PL.Policy.validate(_Eng(), 2, bins, 1.0)
    for rng in (0.0, -1.0, float("nan"), float("inf"), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), "wide", None, (1.0,)):
        with pytest.raises(ValueError):
            PL.policy_bin_edges(rng, 4)
        with pytest.raises(ValueError):
            PL.Policy.validate(_Eng(), 2, 4, rng)
    with pytest.raises(ValueError):
        PL.Policy.validate(_Eng(), -1, 4, 1.0)
    assert PL.Policy.validate(_Eng(), 0, 0, None)[0] == 0           # not asked for: nothing is checked
    assert PL.Policy.validate(_Eng(), 3, 8, 0.5) == (3, 8, (-0.5, 0.5))
    assert PL.Policy.validate(_Eng(), 3, 8, (-1, 2)) == (3, 8, (-1.0, 2.0))
    persistent = _Eng()
    persistent.persistent = True
    with pytest.raises(ValueError, match="persistent"):
        PL.Policy.validate(persistent, 2, 8, 0.5)
    Q, S, z = _case(3, 0)
    with pytest.raises(ValueError):
        PL.host_policy_record(Q, S, z, 4, PL.policy_bin_edges(1.0, 5))
    with pytest.raises(ValueError):
        PL.host_policy_record(Q[:2], S, z, 4, PL.policy_bin_edges(1.0, 4))


def test_datasets_reach_both_sinks(tmp_path, monkeypatch):
    """write_datasets puts the policy datasets after the dwell datasets, through the HDF5 writer and
    the .npz sink alike."""
    from spgg_amd import h5io, spgg
    rs = np.random.RandomState(4)
    L, bins, m = 4, 3, 2
    hist = {name: np.zeros(0) for name in spgg.HISTORY_DATASETS}
    hist.update({f"group_comp_d{d}_history": np.zeros(0) for d in range(6)})
    hist.update({f"{g}_q_{s}_{a}_history": np.zeros(0) for g in ("cooperators", "defectors", "avg") for s in ("s0", "s1") for a in "cd"})
    ph = dict(policy_history_iters=np.arange(1, m + 1), policy_count_history=rs.randint(0, 9, (m, 4, 2, 2)),
              policy_bond_history=rs.randint(0, 9, (m, 5)), policy_gap_hist_history=rs.randint(0, 9, (m, 2, 2, bins + 2)),
              policy_gap_bin_edges=PL.policy_bin_edges(0.5, bins), policy_map_final=rs.randint(0, 16, (L, L)).astype(np.uint8))
    S, Rn = rs.randint(0, 2, (L, L)), np.zeros((L, L))
    for sink in ("npz",) + (("native",) if h5io.h5native.available() else ()):
        monkeypatch.setenv("SPGG_H5_SINK", sink)
        fn = str(tmp_path / f"{sink}.h5")
        spgg.write_datasets(fn, hist, {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64), records=dict(policy=ph))
        got = h5io.read_datasets(fn)
        for name, want in ph.items():
            assert np.array_equal(got[name], want), (sink, name)
            assert got[name].dtype == (np.float64 if name == "policy_gap_bin_edges" else np.uint8 if name == "policy_map_final"
                                       else np.int64), (sink, name)
        names = list(got)
        if sink == "npz":
            assert names[-6:] == list(PL.POLICY_DATASETS) + ["policy_map_final"], names[-8:]
        spgg.write_datasets(fn, hist, {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64))
        assert not set(ph) & set(h5io.read_datasets(fn))


def test_policy_kernels_use_no_scratch():
    if not os.path.exists(KR.LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not available")
    ks = {k: v for k, v in KR._kernels(KR.LIB).items() if "spgg_policy" in k}
    assert len([k for k in ks if "spgg_policy_kernel" in k]) == 4, sorted(ks)      # M = 1 / 2 x one / two tables
    assert any("spgg_policy_bonds_kernel" in k for k in ks) and any("spgg_policy_zero_kernel" in k for k in ks)
    bad = {k: v for k, v in ks.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"] or v["sgpr_spill_count"]}
    assert not bad, bad
    print({k: v["vgpr_count"] for k, v in ks.items()})
