"""The payoff record on the CPU: the payoff table against the oracle within a derived bound, the census
against the oracle's group-composition counts and payoff sums, the host model against a literal
per-agent loop and its invariants, the NumPy model of the device's pair-sum scheme against np.roll, the
ABI's three statements of the new entry points, the option tables, the dataset writers and the built
kernels' register budget.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import spgg_oracle as O
from spgg_amd import _lib, payoff as PF, records
from tests import _payoff as K
from tests import test_kernel_resources_cpu as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "spgg_abi.h")


def _lattices():
    rs = np.random.RandomState(77)
    for L in K.CHECK_SIDES:
        for dens in K.CHECK_DENSITIES:
            yield L, (rs.rand(L, L) < dens).astype(np.int64)


# ---- the table and the census against the oracle ----------------------------------------------------------------
def test_payoff_values_against_the_oracle():
    """payoff_values(p)[sigma, K] is oracle.payoff at every agent, within tests/_payoff.value_bound."""
    worst = 0.0
    rows = K.oracle_rows()
    assert len(rows) >= len(K.CHECK_ROWS) + 20
    reached = np.zeros((2, 26), dtype=bool)
    for L, S in _lattices():
        sigma, _m, Kf = PF.payoff_fields(S)
        reached[sigma, Kf] = True
        for p in rows:
            want, got = O.payoff(S, p), PF.payoff_values(p)[sigma, Kf]
            bound = K.value_bound(p, Kf)
            err = np.abs(got - want)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (L, p.r, p.c, p.cost, float((err / bound).max()))
    print("largest error in units of the bound:", worst)
    assert 0 < worst           # the two expressions do round differently: the bound is not vacuous
    assert reached[0, 5:].all() and not reached[0, :5].any()         # cooperators: K = 5 .. 25
    assert reached[1, :21].all() and not reached[1, 21:].any()       # defectors: K = 0 .. 20
    assert PF.payoff_values(dict(r=2.0, c=1.0, cost=0.5)).shape == (2, 26)
    assert np.array_equal(PF.payoff_values(dict(r=2.0, c=1.0, cost=0.5)), PF.payoff_values(O.Params()))


def test_census_marginals_and_sums_against_the_oracle():
    for L, S in _lattices():
        row, _plane = PF.host_payoff_census(S)
        census = PF.split_census(row)[0]
        sigma, _m, Kf = PF.payoff_fields(S)
        # the agents whose own group holds d defectors: d = 5 - N = 5 - (c + m)
        nd = O.sum5((S == 1).astype(int))
        want = np.bincount(nd.ravel(), minlength=6)
        got = np.zeros(6, dtype=np.int64)
        for sg in (0, 1):
            for m in range(5):
                got[5 - ((1 - sg) + m)] += census[sg, m].sum()
        assert np.array_equal(got, want), (L, got, want)
        for p in K.oracle_rows():
            P = O.payoff(S, p)
            V = PF.payoff_values(p)
            by = census.sum(axis=1)
            for mask, mine in ((np.ones_like(S, dtype=bool), (by * V).sum()), (S == 0, (by[0] * V[0]).sum()),
                               (S == 1, (by[1] * V[1]).sum())):
                want_sum = np.sum(P[mask])
                bound = K.sum_bound(p, Kf[mask], float(np.abs(P[mask]).sum())) if mask.any() else 0.0
                assert abs(mine - want_sum) <= bound, (L, p.r, mine, want_sum, bound)


# ---- the host model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7])
def test_host_model_against_a_literal_loop(L):
    for name, S in K.patterns(L).items():
        row, plane = PF.host_payoff_census(K.dirty(S, L))            # the bookkeeping bits change nothing
        want, want_plane = K.literal_census(S)
        assert row.dtype == np.int64 and plane.dtype == np.uint8 and row.shape == (K.SLOTS,)
        assert np.array_equal(row, want), (L, name, np.nonzero(row != want)[0].tolist())
        assert np.array_equal(plane, want_plane), (L, name)


@pytest.mark.parametrize("L", [2, 5, 13, 18])
def test_invariants(L):
    n = L * L
    for name, S in K.patterns(L).items():
        row, plane = PF.host_payoff_census(S)
        census, cd, cc, dd = PF.split_census(row)
        assert census.sum() == n and cd.sum() + cc.sum() + dd.sum() == 2 * n, name
        assert census[0].sum() == np.count_nonzero(S == 0)
        sigma, m, Kf = PF.payoff_fields(S)
        assert np.array_equal(plane & 31, Kf) and np.array_equal(plane >> 5 & 1, sigma) and np.array_equal(plane >> 6, m & 3)
        # transposing the lattice swaps "right" and "lower": the bond rows are those of both together
        assert np.array_equal(PF.host_payoff_census(S.T)[0], row), name
        # the left and the upper neighbour instead of the right and the lower one: the same bonds
        other = PF.host_payoff_census(S[::-1, ::-1])[0]
        assert np.array_equal(other, row), name
        D = L // 2
        pr = PF.host_payoff_pairs(S)
        sK, sc, rows, cols = PF.split_pairs(pr, D)
        hc = records.host_pair_counts(S, D)
        assert np.array_equal(rows[:, 2], hc[0]) and np.array_equal(cols[:, 2], hc[1]), name      # CC: spgg_correlations' counts
        assert rows[0, 0] == cols[0, 0] == (Kf * Kf).sum() and sK == Kf.sum() == 25 * sc          # every cooperator is counted 25 times
        assert rows[0, 1] == 2 * (Kf * (1 - sigma)).sum()
        assert np.array_equal(PF.host_payoff_pairs(S, 0), pr[[0, 1, 2, 3, 4, 2 + 3 * (D + 1), 3 + 3 * (D + 1), 4 + 3 * (D + 1)]])
    with pytest.raises(ValueError):
        PF.host_payoff_pairs(np.zeros((4, 4)), 3)
    with pytest.raises(ValueError):
        PF.host_payoff_census(np.zeros((4, 5)))


def test_reachable_slots():
    """Which census slots can hold an agent.  A cooperator with m cooperating neighbours has N = 1 + m at its
    own cell; a cooperating neighbour's N lies in 2 .. 5 (itself and the agent), a defecting one's in 1 .. 4:
    K in 5 + 2 m .. 17 + 2 m.  A defector has N = m; a cooperating neighbour's N lies in 1 .. 4, a defecting
    one's in 0 .. 3: K in 2 m .. 12 + 2 m.  That is 13 totals for each of the ten (sigma, m): 130 slots, and
    random lattices reach every one of them; the others stay zero."""
    total = np.zeros(K.SLOTS, dtype=np.int64)
    rs = np.random.RandomState(5)
    for L in K.CHECK_SIDES:
        for dens in K.CHECK_DENSITIES:
            for _ in range(8):
                total += PF.host_payoff_census((rs.rand(L, L) < dens).astype(np.int64))[0]
    census, cd, cc, dd = PF.split_census(total)
    print(np.count_nonzero(census), np.nonzero(cd)[0][[0, -1]] - 25, np.nonzero(cc)[0][-1], np.nonzero(dd)[0][-1])
    may = np.zeros((2, 5, 26), dtype=bool)
    for m in range(5):
        may[0, m, 5 + 2 * m:17 + 2 * m + 1] = True
        may[1, m, 2 * m:12 + 2 * m + 1] = True
    assert may.sum() == 130 and np.array_equal(census > 0, may)
    # K weighs the cells around an agent 5 (itself), 2 (the eight cells next to it), 1 (two steps along an
    # axis).  The weights of two neighbouring agents differ by +3 / -3 at the two agents themselves and by
    # +-8 in all elsewhere: a like bond has |dK| <= 8, a C-D bond K_C - K_D in 3 - 8 .. 3 + 8.
    assert np.nonzero(cd)[0][0] == 25 - 5 and np.nonzero(cd)[0][-1] == 25 + 11
    assert np.nonzero(cc)[0][-1] == 8 and np.nonzero(dd)[0][-1] == 8


def test_derived_quantities():
    S = K.patterns(13)["density_0.5"]
    row = PF.host_payoff_census(S)[0]
    p = O.Params(r=3.0, c=1.0, cost=0.5)
    P = O.payoff(S, p)
    for strategy, mask in ((None, np.ones_like(S, dtype=bool)), (0, S == 0), (1, S == 1)):
        vals, counts = PF.payoff_distribution(row, p, strategy)
        assert counts.sum() == mask.sum() and np.all(np.diff(vals) >= 0) and np.all(counts > 0)
        assert abs((vals * counts).sum() - P[mask].sum()) < 1e-9
        x = np.sort(P[mask])
        n = x.size
        want = ((2 * np.arange(1, n + 1) - n - 1) * x).sum() / (n * x.sum())          # the sorted-sample formula
        assert abs(PF.gini(vals, counts) - want) < 1e-9
    assert np.isnan(PF.gini([], [])) and PF.gini([1.0, 1.0], [3, 4]) == 0.0
    more, same, less = PF.interface_advantage(row, p)
    sigma, _m, Kf = PF.payoff_fields(S)
    gaps = []
    for axis in (1, 0):
        s2, P2 = np.roll(sigma, -1, axis=axis), np.roll(P, -1, axis=axis)
        cd = sigma != s2
        gaps.append(np.where(sigma == 0, P - P2, P2 - P)[cd])
    g = np.concatenate(gaps)
    tie = np.abs(g) < 1e-12
    assert abs(more - np.mean((g > 0) & ~tie)) < 1e-12 and abs(less - np.mean((g < 0) & ~tie)) < 1e-12 and abs(same - tie.mean()) < 1e-12
    assert all(np.isnan(v) for v in PF.interface_advantage(PF.host_payoff_census(np.zeros((4, 4)))[0], p))
    # r c dK / 5 = 5 cost at dK = 5: the cooperator earns the same
    tie_p = dict(r=2.0, c=1.0, cost=0.4)
    cd = PF.split_census(row)[1]
    assert cd[30] > 0 and PF.interface_advantage(row, tie_p)[1] == cd[30] / cd.sum()
    # ties in real arithmetic whose doubles are not: 3 * 5 / 5 = 5 * 0.6, 0.7 * 1.5 * 5 / 5 = 5 * 0.21
    for p_, dK in ((dict(r=3.0, c=1.0, cost=0.6), 5), (dict(r=0.7, c=1.5, cost=0.21), 5), (dict(r=0.3, c=1.0, cost=0.06), 5),
                   (dict(r=1.1, c=1.0, cost=0.132), 3)):
        more_, same_, less_ = PF.interface_advantage(row, p_)
        assert cd[25 + dK] > 0 and same_ == cd[25 + dK] / cd.sum(), (p_, same_)
        assert abs(more_ - cd[25 + dK + 1:].sum() / cd.sum()) < 1e-15 and abs(more_ + same_ + less_ - 1) < 1e-15
    near = dict(r=3.0, c=1.0, cost=0.6 * (1 + 2.0 ** -40))             # not a tie: far outside the tolerance
    assert PF.interface_advantage(row, near)[1] == 0.0
    D = 6
    G = PF.payoff_correlation_function(PF.host_payoff_pairs(S, D), S.size, p)
    want = [(np.mean(P * np.roll(P, -d, axis=1)) + np.mean(P * np.roll(P, -d, axis=0))) / 2 - P.mean() ** 2 for d in range(D + 1)]
    assert G.shape == (D + 1,) and np.allclose(G, want, rtol=0, atol=1e-12)
    assert abs(G[0] - P.var()) < 1e-12


# ---- the NumPy model of the device's pair-sum scheme ------------------------------------------------------------------
SIDES = [1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 33, 64, 65, 200, 201]     # tests/test_reputation_cpu.py's


def _planes(L):
    pats = K.patterns(L)
    return {name: PF.host_payoff_census(K.dirty(pats[name], L))[1] for name in K.PATTERN_NAMES}


@pytest.mark.parametrize("L", SIDES)
def test_rotation_model_equals_roll(L):
    for name, plane in _planes(L).items():
        Kf, c = (plane & 31).astype(np.int64), 1 - (plane >> 5 & 1).astype(np.int64)
        for d in range(L // 2 + 1):
            mk, mc = K.model_rotate(plane, d)
            assert np.array_equal(mk, np.roll(Kf, -d, axis=1)) and np.array_equal(mc, np.roll(c, -d, axis=1)), (L, name, d)
    q = K.staged(next(iter(_planes(L).values())))
    pad = np.ascontiguousarray(q).view(np.uint8).reshape(L, -1)[:, L:]
    assert not pad.any()                  # the zero padding: no cooperator, no K beyond the row


@pytest.mark.parametrize("L", SIDES)
def test_pair_sum_model_equals_definition(L):
    for name, plane in _planes(L).items():
        D = L // 2
        strategies = plane >> 5 & 1
        assert np.array_equal(K.model_pairs(plane, D), PF.host_payoff_pairs(strategies, D)), (L, name)


def test_lane_bounds():
    """The static_asserts of csrc/spgg_payoff.h, restated: the int32 lane partials at the largest sides."""
    assert K.LANE_DOTS_MAX == 858993 and K.LANE_DOTS_MAX * K.DOT_MAX < 2 ** 31 <= (K.LANE_DOTS_MAX + 1) * K.DOT_MAX
    assert K.max_side() == 46340 and K.lane_dots_global(46340) == 2897 * 182 <= K.LANE_DOTS_MAX
    W = (404 + 3) // 4
    assert 404 * W * 4 <= 163840 < 405 * ((405 + 3) // 4) * 4           # 404: the last side staged in LDS
    assert max(404 * ((W + 63) // 64), (404 * W + 63) // 64) <= K.LANE_DOTS_MAX
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    side = ctypes.c_int32(-5)
    assert _lib.load().spgg_payoff_pairs_max_side(None, ctypes.byref(side)) == _lib.OK and side.value == K.max_side()
    assert _lib.load().spgg_payoff_pairs_max_side(None, None) == _lib.E_ARG


# ---- header, binding, exports, option tables ------------------------------------------------------------------------------
NEW = ("spgg_payoff_census", "spgg_payoff_pairs", "spgg_payoff_pairs_max_side")


def test_header_binding_and_exports_agree():
    text = open(HEADER).read()
    assert int(re.search(r"#define SPGG_ABI_VERSION (\d+)", text).group(1)) == 19 == _lib.ABI_VERSION
    for name, value in (("SLOTS", _lib.PAYOFF_SLOTS), ("BOND_CD", _lib.PAYOFF_BOND_CD), ("BOND_CC", _lib.PAYOFF_BOND_CC),
                        ("BOND_DD", _lib.PAYOFF_BOND_DD)):
        assert int(re.search(rf"#define SPGG_PAYOFF_{name} (\d+)", text).group(1)) == value, name
    assert (_lib.PAYOFF_SLOTS, _lib.PAYOFF_BOND_CD, _lib.PAYOFF_BOND_CC, _lib.PAYOFF_BOND_DD) == (K.SLOTS, K.BOND_CD, K.BOND_CC, K.BOND_DD)
    assert (K.BOND_CD, K.BOND_CC - K.BOND_CD, K.BOND_DD - K.BOND_CC, K.SLOTS - K.BOND_DD) == (2 * 5 * 26, 51, 26, 26)
    names = {"spgg_payoff_census": ["ctx", "t", "plane", "out", "out_stride", "hip_stream"],
             "spgg_payoff_pairs": ["ctx", "t", "max_d", "plane", "out", "out_stride", "hip_stream"],
             "spgg_payoff_pairs_max_side": ["ctx", "side"]}
    for fn, want in names.items():
        proto = re.search(rf"int {fn}\(([^)]*)\);", text).group(1)
        args = [a.strip().split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
        assert args == want and fn in _lib.EXPORTED, fn
    assert PF.pairs_width(0) == 8 and PF.pairs_width(4) == 32
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libspgg_hip.so not built")
    lib = _lib.load()
    assert lib.spgg_abi_version() == 19
    for fn, want in names.items():
        f = getattr(lib, fn)
        assert f.restype is ctypes.c_int and len(f.argtypes) == len(want), fn
    assert lib.spgg_payoff_census(None, 1, None, None, K.SLOTS, None) == _lib.E_ARG          # a null context
    assert lib.spgg_payoff_pairs(None, 1, 0, None, None, 8, None) == _lib.E_ARG


def test_option_tables():
    from spgg_amd import spgg, sweep
    """The payoff options through the one entry point (the table itself: tests/test_records_cpu.py)."""
    mine = ["payoff_history_every", "payoff_max_distance", "payoff_map_final"]

    def values(v):
        run_kw, extras = spgg.record_options(v)
        return {k: x for k, x in run_kw.items() if k.startswith("payoff")}, extras["payoff_map_final"]

    assert [o[0] for o in PF.Payoff.options] == mine
    assert (spgg.SPGG.payoff_history_every, spgg.SPGG.payoff_max_distance, spgg.SPGG.payoff_map_final) == (0, None, False)
    kw = dict(L=8, payoff_history_every="3", payoff_max_distance=2, payoff_map_final=1, epsilon=0.2)
    got = {k: v for k, v in sweep.pop_record_options(kw).items() if k in mine}
    assert got == dict(payoff_history_every=3, payoff_max_distance=2, payoff_map_final=True) and kw == dict(L=8, epsilon=0.2)
    assert {k: v for k, v in sweep.pop_record_options({}).items() if k in mine} == {o[0]: o[2] for o in PF.Payoff.options}
    assert values(got) == (dict(payoff_every=3, payoff_max_d=2), True)
    assert values({}) == (dict(payoff_every=0, payoff_max_d=None), False)
    for bad in (dict(payoff_map_final=True), dict(payoff_max_distance=2)):
        with pytest.raises(ValueError, match="payoff_max_distance and payoff_map_final need payoff_history_every > 0"):
            values(bad)
    assert records.KINDS["payoff"] is PF.Payoff and issubclass(PF.Payoff, records.Record)
    assert PF.PAYOFF_DATASETS == ("payoff_history_iters", "payoff_census_history", "payoff_bond_history", "payoff_values")


class _Eng:
    L, payoff_pairs_max_side, persistent = 18, 46340, True


def test_every_value_error():
    assert PF.Payoff.validate(_Eng(), 0, None) == (0, None)
    with pytest.raises(ValueError, match="payoff_every"):
        PF.Payoff.validate(_Eng(), 0, 4)                              # a distance without the record, as the option layer
    assert PF.Payoff.validate(_Eng(), 3, None) == (3, None) and PF.Payoff.validate(_Eng(), "3", 9) == (3, 9)
    for every, D in ((-1, None), (2, -1), (2, 10)):
        with pytest.raises(ValueError):
            PF.Payoff.validate(_Eng(), every, D)
    wide = _Eng()
    wide.L, wide.payoff_pairs_max_side = 500, 404
    with pytest.raises(ValueError, match="404"):
        PF.Payoff.validate(wide, 2, 3)
    assert PF.Payoff.validate(wide, 2, None) == (2, None)            # the census has no side limit


def test_datasets_reach_both_sinks(tmp_path, monkeypatch):
    """write_datasets puts the payoff datasets after the policy datasets, through the HDF5 writer and the
    .npz sink alike; without the record the file holds the set it held before."""
    from spgg_amd import h5io, spgg
    rs = np.random.RandomState(4)
    L, m, D = 4, 2, 1
    hist = {name: np.zeros(0) for name in spgg.HISTORY_DATASETS}
    hist.update({f"group_comp_d{d}_history": np.zeros(0) for d in range(6)})
    hist.update({f"{g}_q_{s}_{a}_history": np.zeros(0) for g in ("cooperators", "defectors", "avg") for s in ("s0", "s1") for a in "cd"})
    base = dict(payoff_history_iters=np.arange(1, m + 1), payoff_census_history=rs.randint(0, 9, (m, 2, 5, 26)),
                payoff_bond_history=rs.randint(0, 9, (m, 103)), payoff_values=PF.payoff_values(O.Params()))
    full = dict(base, payoff_pair_sums_history=rs.randint(0, 9, (m, PF.pairs_width(D))),
                payoff_map_final=rs.randint(0, 256, (L, L)).astype(np.uint8))
    S, Rn = rs.randint(0, 2, (L, L)), np.zeros((L, L))
    for sink in ("npz",) + (("native",) if h5io.h5native.available() else ()):
        monkeypatch.setenv("SPGG_H5_SINK", sink)
        fn = str(tmp_path / f"{sink}.h5")
        spgg.write_datasets(fn, hist, {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64))
        plain = list(h5io.read_datasets(fn))
        assert not set(full) & set(plain)
        for ph in (base, full):
            spgg.write_datasets(fn, hist, {}, S, Rn, -10, 10, [], clusters=np.zeros(0, dtype=np.int64), records=dict(payoff=ph))
            got = h5io.read_datasets(fn)
            for name, want in ph.items():
                assert np.array_equal(got[name], want), (sink, name)
                assert got[name].dtype == (np.float64 if name == "payoff_values" else np.uint8 if name == "payoff_map_final"
                                           else np.int64), (sink, name)
            assert set(got) == set(plain) | set(ph), sink
            if sink == "npz":
                assert list(got) == plain + list(ph), list(got)[-8:]


def test_payoff_kernels_use_no_scratch():
    if not os.path.exists(KR.LIB):
        pytest.skip("libspgg_hip.so not built")
    if not os.path.exists(KR.READELF):
        pytest.skip("llvm-readelf not available")
    ks = {k: v for k, v in KR._kernels(KR.LIB).items() if "spgg_pf" in k}
    for part, count in (("spgg_payoff_zero_kernel", 1), ("spgg_payoff_census_kernel", 1), ("spgg_payoff_pairs_lds_kernel", 2),
                        ("spgg_payoff_pairs_global_kernel", 1)):
        assert len([k for k in ks if part in k]) == count, (part, sorted(ks))
    assert len(ks) == 5, sorted(ks)
    bad = {k: v for k, v in ks.items() if v["private_segment_fixed_size"] or v["vgpr_spill_count"] or v["sgpr_spill_count"]}
    assert not bad, bad
    print({k: v["vgpr_count"] for k, v in ks.items()})
