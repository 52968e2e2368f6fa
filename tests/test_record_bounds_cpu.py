"""The exact history record (tests/_record.py) and its bounds, checked without a GPU.

1. exact_record() through histories_from_stats reproduces the reference's datasets for every golden
   case, at test_host_histories.py's bar.
2. The reference alone stays inside the bounds: NumPy models of what the device executes -- the f64
   summation order (agents per thread, the wave's tree, four waves, tiles in a shuffled order onto
   stripes), spgg_history_finalize_kernel's regrouped formulas, the f32 NI chain with v_rcp_f32 taken
   as an exact reciprocal moved one ulp either way -- hold them at every lattice the GPU file runs.
3. Sensitivity, the condition that makes the GPU test worth having: one agent's term lost from (or
   counted twice in) a sum moves it by far more than the slot's bound.
"""
import functools
import types

import numpy as np
import pytest

from oracle import spgg_oracle as O
from spgg_amd.engine import epsilon_table, histories_from_stats
from tests import _params as P
from tests import _record as R
from tests._golden import Case, case_names

# the datasets held bit for bit (as tests/test_host_histories.py)
EXACT = {"coop_rate_history", "switch_C_to_D", "switch_D_to_C", "epsilon_history_final",
         "best_neighbor_second_order_percent"} | {f"group_comp_d{d}_history" for d in range(6)}
T_CPU = 4       # executed steps per lattice here (the bounds are per slot: more steps check nothing new)


# ---- 1. the exact record reproduces the reference's datasets -----------------------------------
@pytest.mark.parametrize("name", case_names())
def test_exact_record_reproduces_reference_datasets(name):
    c = Case(name)
    p = c.oracle_params()
    rs = np.random.RandomState(c.seed)
    Q, tables = O.init_tables(p, rs)
    S = rs.randint(0, 2, size=(p.L, p.L)) if c.S_in_one is None else c.S_in_one
    rec = R.exact_record(p, p.L, p.iterations, p.use_second_order, p.state_representation, p.algorithm, rs=rs,
                         init=types.SimpleNamespace(Q=Q, S=S, tables=tables))
    eps = epsilon_table(p.epsilon, p.epsilon_decay, p.epsilon_min, p.iterations + 1)
    got = histories_from_stats(rec.value, rec.last, rec.stop_iter != 0, eps, rec.n)
    want = {k: v for k, v in c.datasets.items() if k in got}
    assert set(got) == set(want)
    for k in want:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype or (g.size == 0 and w.size == 0), k
        if k in EXACT:
            assert np.array_equal(g, w, equal_nan=True), k
        else:
            np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-15, equal_nan=True, err_msg=k)
    # nothing outside the executed iterations
    assert not rec.value[rec.last + 2:].any() and not rec.value[0, :R.GC0].any()


# ---- the lattices of tests/test_gpu_record.py, one oracle run each (read only) ------------------
VARIANTS = {L: [("qlearning", L != 1000 and L != 200, 1.0)] for L in list(R.GPU_LATTICES) + [200]}
VARIANTS[18].append(("double_qlearning", True, 1.0))
VARIANTS[60].append(("sarsa", True, 0.3))                # non-dyadic gain: the f64 reputation path
VARIANTS[120].append(("double_qlearning", False, 0.3))
VARIANTS[120].append(("expected_sarsa", False, 0.3))
CASES = [(L, alg, M2, gain) for L in sorted(VARIANTS) for alg, M2, gain in VARIANTS[L]]
TILES = dict(R.GPU_LATTICES)
TILES[200] = (40, 25, 4, 1)
# The rows the parameter-space tests step (tests/_params.py: all but the payoff-only ones) at L = 18;
# the last element of a case is then the row's name.
ROWS = {k: v for k, v in P.all_rows().items() if not k.startswith("a-")}
ROW_CASES = [(18, "qlearning", True, name) for name in sorted(ROWS)]
ROW_CASES += [(18, "double_qlearning", True, name) for name in sorted(ROWS) if name.startswith("b-dyadic")]
ALL_CASES = CASES + ROW_CASES


@functools.lru_cache(maxsize=None)
def _rec(L, alg, M2, gain):
    T = 3 if L >= 200 else T_CPU
    params = ROWS[gain] if isinstance(gain, str) else dict(R.BASE, rep_gain_C=gain, r=3.4)
    return R.philox_record(L, T, params, 5, 0, M2, "reputation", alg, keep_terms=True)


def _dyadic(gain):
    return P.unit_of(ROWS[gain]) is not None if isinstance(gain, str) else gain == 1.0


def _steps(rec):
    return range(1, (rec.last - 1 if rec.stop_iter else rec.last) + 1)


# ---- 2a. the device's f64 summation order -------------------------------------------------------
def tile_totals(x, tile, f32_threads=False):
    """Workgroup totals of the (L, L) grid x of masked per-agent terms (0 where masked), as the step
    kernel forms them: tiles of tw x th cells (cells past the lattice edge and the slots past the
    tile are invalid: 0), slot s of a tile in thread s % 256 as its agent s // 256; each thread adds
    its agents in turn (f32_threads: in f32, the NI percent), the wave's 64 lanes meet in a binary
    tree, the four wave totals are added in order."""
    tw, th, apt, _ = tile
    L = x.shape[0]
    assert tw * th <= 256 * apt
    ny, nx = -(-L // th), -(-L // tw)
    pad = np.zeros((ny * th, nx * tw), dtype=x.dtype)
    pad[:L, :L] = x
    cells = pad.reshape(ny, th, nx, tw).transpose(0, 2, 1, 3).reshape(ny * nx, th * tw)
    slots = np.zeros((ny * nx, 256 * apt), dtype=x.dtype)
    slots[:, :th * tw] = cells
    slots = slots.reshape(ny * nx, apt, 256)
    acc = np.zeros((ny * nx, 256), dtype=np.float32 if f32_threads else np.float64)
    for u in range(apt):
        acc = acc + slots[:, u, :]
    w = acc.astype(np.float64).reshape(ny * nx, 4, 64)
    h = 32
    while h:
        w = w[..., :h] + w[..., h:2 * h]
        h //= 2
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def fold(totals, stripes, rng):
    """The workgroups' atomicAdds onto stripe tile % stripes in a shuffled order, then the stripes."""
    acc = [0.0] * stripes
    for i in rng.permutation(len(totals)):
        acc[i % stripes] += float(totals[i])
    out = 0.0
    for a in acc:
        out += a
    return out


def model_f64_slots(rec, t, tile, rng):
    """{slot: value} of the f64 accumulated slots of step t in the device's order."""
    g = rec.terms[(t, "grids")]
    pc = (g["prev_S"] == 0).astype(np.float64)
    ac = (g["actions"] == 0).astype(np.float64)
    st = tile[3]
    out = {R.SUMR: fold(tile_totals(g["R"], tile), st, rng),
           R.SUM_REW_C: fold(tile_totals(g["rew"] * ac, tile), st, rng)}
    for e in range(4):
        q = g["Q"][:, :, e // 2, e % 2]
        tot, tot_c = tile_totals(q, tile), tile_totals(q * pc, tile)
        out[R.SUMQ + e] = fold(tot, st, rng)
        out[R.SUMQ_C + e] = fold(tot_c, st, rng)
        out[R.SUMQ_D + e] = fold(tot - tot_c, st, rng)        # epilogue: total - C per workgroup
    return out


def model_ratio(rec, t, tile, rng, ulps):
    """SUM_RATIO_C with rcp_diag taken as the rounded reciprocal moved `ulps` ulps."""
    g = rec.terms[(t, "grids")]
    rcp = 1.0 / (np.abs(g["rew"]) + 1e-9)
    for _ in range(abs(ulps)):
        rcp = np.nextafter(rcp, np.inf if ulps > 0 else -np.inf)
    term = (np.abs(g["wr"]) * rcp) * (g["actions"] == 0)
    return fold(tile_totals(term, tile) * 100.0, tile[3], rng)


def _check_f64(rec, L, steps):
    b = R.bounds(rec)
    rng = np.random.RandomState(L)
    for t in steps:
        got = model_f64_slots(rec, t, TILES[L], rng)
        for ulps in (-1, 0, 1):
            got[(R.SUM_RATIO_C, ulps)] = model_ratio(rec, t, TILES[L], rng, ulps)
        for k, v in got.items():
            k = k[0] if isinstance(k, tuple) else k
            err = abs(v - rec.value[t, k])
            assert err <= b[t, k], (t, R.SLOT_NAMES[k], v, rec.value[t, k], b[t, k])


@pytest.mark.parametrize("L,alg,M2,gain", ALL_CASES)
def test_reference_in_device_order_stays_inside_f64_bounds(L, alg, M2, gain):
    rec = _rec(L, alg, M2, gain)
    assert rec.rep_dyadic == _dyadic(gain)
    _check_f64(rec, L, _steps(rec))


def test_int8_reputation_sum_is_representable():
    """SUMR on the int8 path is an integer sum of R / unit times the dyadic unit: exact while
    |k| * n < 2^53, at every lattice used (|k| <= 127)."""
    for L in R.GPU_LATTICES:
        assert 127 * L * L < 2 ** 53
    rec = _rec(1000, "qlearning", False, 1.0)
    assert rec.rep_dyadic and rec.rep_units_max < 2.0 ** 53
    assert not R.bounds(rec)[:, R.SUMR].any()


# ---- 2b. the finalize kernel's regrouped formulas ------------------------------------------------
def model_finalize(p, gc, nc, nc1, n, sw_cd, rew_c):
    """spgg_history_finalize_kernel in Python floats (the same f64 operations in its order)."""
    rc = p.r * p.c
    pay_c = [rc * N / 5 - p.cost for N in range(6)]
    pay_d = [rc * N / 5 for N in range(6)]
    norm_min, norm_den = p.r - 5, 4 * p.r - (p.r - 5)
    w_p, w_rep = float(p.reward_weight_payoff), float(1 - p.reward_weight_payoff)
    praw = praw_c = 0.0
    for d in range(6):
        praw_c += gc[d] * ((5 - d) * pay_c[5 - d])
        praw += gc[d] * ((5 - d) * pay_c[5 - d] + d * pay_d[5 - d])
    sump = (praw - n * norm_min) / norm_den
    sump_c = (praw_c - nc * norm_min) / norm_den
    wpp = w_p * sump
    wrr = nc1 * (w_rep * 0.5)
    return {R.SUMP: sump, R.SUMP_C: sump_c, R.SUMP_D: sump - sump_c, R.SUM_WPP: wpp, R.SUM_WRR: wrr,
            R.SUM_REW_D: (wpp + wrr) - rew_c, R.SW_DC: sw_cd + nc1 - nc}


def _check_finalize(rec, rew_c_of, steps=None):
    b = R.bounds(rec)
    v = rec.value
    for t in _steps(rec) if steps is None else steps:
        got = model_finalize(rec.params, v[t - 1, R.GC0:R.GC0 + 6], v[t, R.NCOOP], v[t + 1, R.NCOOP], rec.n,
                             v[t, R.SW_CD], rew_c_of(t))
        for k, x in got.items():
            assert abs(x - v[t, k]) <= b[t, k], (t, R.SLOT_NAMES[k], x, v[t, k], b[t, k])
        assert got[R.SUM_WRR] == v[t, R.SUM_WRR] and got[R.SW_DC] == v[t, R.SW_DC]


@pytest.mark.parametrize("L,alg,M2,gain", ALL_CASES)
def test_regrouped_slots_stay_inside_bounds(L, alg, M2, gain):
    rec = _rec(L, alg, M2, gain)
    rng = np.random.RandomState(L + 1)
    _check_finalize(rec, lambda t: model_f64_slots(rec, t, TILES[L], rng)[R.SUM_REW_C])


@pytest.mark.parametrize("r", [0.7, 3.0, 4.999, 6.5])
@pytest.mark.parametrize("w_p", [0.5, 0.95, 1.0])
def test_regrouped_slots_over_payoff_parameters(r, w_p):
    """Synergy factors around the normalisation's r - 5 = 0 and pay_c's sign change, and payoff
    weights with and without a reputation reward."""
    rec = R.philox_record(24, 6, dict(R.BASE, r=r, reward_weight_payoff=w_p), 3, 0, False, "reputation")
    _check_finalize(rec, lambda t: rec.value[t, R.SUM_REW_C])
    if w_p == 1.0:      # slots the parameters force to zero
        assert not rec.value[:, R.SUM_WRR].any() and not rec.value[:, R.SUM_RATIO_C].any()
        assert not R.bounds(rec)[:, [R.SUM_WRR, R.SUM_RATIO_C]].any()


# ---- 2c. the f32 NI chain ----------------------------------------------------------------------
def model_pct(rec, t, tile, rng, ulps):
    """SUM_PCT as phase 1a forms it: float casts, two f32 additions, the reciprocal (rounded, then
    moved `ulps` ulps), the product, fmaf accumulation per thread, f64 from there, * 100 per tile."""
    g = rec.terms[(t, "grids")]
    f = np.float32
    anu = np.abs(g["nu"].astype(f))
    atd = g["atd2"].astype(f)
    rcp = f(1.0) / ((atd + anu) + f(1e-8))
    if ulps:
        rcp = np.nextafter(rcp, f(np.inf if ulps > 0 else -np.inf))
    term = anu * rcp
    assert term.dtype == f
    return fold(tile_totals(term, tile, f32_threads=True) * 100.0, tile[3], rng)


@pytest.mark.parametrize("L,alg,M2,gain", ALL_CASES)
def test_reference_in_f32_chain_stays_inside_pct_bound(L, alg, M2, gain):
    rec = _rec(L, alg, M2, gain)
    _check_pct(rec, L, _steps(rec))


def _check_pct(rec, L, steps):
    b = R.bounds(rec)
    rng = np.random.RandomState(L + 2)
    for t in steps:
        if rec.params.influence_factor == 0.0:      # nu = +0: the slot and its bound are exactly 0
            assert rec.value[t, R.SUM_PCT] == 0.0 and b[t, R.SUM_PCT] == 0.0
        else:
            assert rec.mag[t, R.SUM_PCT] > 0
        for ulps in (-1, 0, 1):
            v = model_pct(rec, t, TILES[L], rng, ulps)
            assert abs(v - rec.value[t, R.SUM_PCT]) <= b[t, R.SUM_PCT], (t, ulps, v, rec.value[t, R.SUM_PCT])


def test_forced_zero_slots_have_zero_bounds():
    rec = R.philox_record(16, 5, dict(R.BASE, influence_factor=0.0, reward_weight_payoff=1.0), 2, 0, True,
                          "reputation")
    b = R.bounds(rec)
    for k in (R.SUM_PCT, R.SUM_RATIO_C, R.SUM_WRR):
        assert not rec.value[:, k].any() and not b[:, k].any()
    assert rec.value[1:rec.last + 1, R.GMAX].all()       # the lattice max does not depend on kappa
    assert not b[rec.last + 1:].any() and not b[0].any()
    assert not b[:, list(R.COUNTERS) + [R.GMAX]].any()


# ---- 3. sensitivity ------------------------------------------------------------------------------
def _median_term(rec, t, k):
    x = np.abs(rec.terms[(t, k)])
    x = x[x != 0]
    return float(np.median(x)) if x.size else None


@pytest.mark.parametrize("L,alg,M2,gain", ALL_CASES)
def test_one_agent_moves_a_sum_by_far_more_than_its_bound(L, alg, M2, gain):
    """Dropping or repeating one agent's median-magnitude non-zero term moves every f64 float slot
    by more than 100 x its bound (a loss is sure to be seen from 2 x on: the honest error is within
    one bound of the exact sum, the faulty one a whole term away from that).

    The f32 NI percent is weaker: at L <= 200 a median term is > 1 x (in fact > 2 x) its bound, so
    a lost agent is seen; at L = 1000 it is NOT: the bound (8 + 4 roundings of 2^-24 on a sum of 10^6
    terms in [0, 100]) is 30 - 35 against a median term of 54 - 65, a ratio of 1.6 - 1.9: below the
    2 x from which a loss is sure to show, and two orders short of the 100 x the f64 slots have.
    SUM_PCT cannot be relied on to see one agent in 10^6 ("Precision of the history
    record")."""
    rec = _rec(L, alg, M2, gain)
    _check_sensitivity(rec, L, _steps(rec))


def _check_sensitivity(rec, L, steps):
    b = R.bounds(rec)
    slots = [k for k in R.F64_SUM_SLOTS + R.REGROUPED if not (k == R.SUMR and rec.rep_dyadic)]
    # slots whose every term the parameters make exactly 0 (their bounds are 0 too: bit-equal on the
    # device): no reputation reward at w_P = 1; 0 * P and a defector's reward 0 * P + w_rep * 0 at w_P = 0
    if rec.params.reward_weight_rep == 0.0:
        slots.remove(R.SUM_RATIO_C)
    if rec.params.reward_weight_payoff == 0.0:
        slots = [k for k in slots if k not in (R.SUM_WPP, R.SUM_REW_D)]
        assert not b[:, R.SUM_WPP].any()
    seen = set()
    for t in steps:
        for k in slots:
            med = _median_term(rec, t, k)
            if med is None:         # (no reputation yet at t = 1: R_1 = 0)
                continue
            seen.add(k)
            if R.SUMQ_D <= k < R.SUMQ_D + 4:
                # the kernel has no prev-D accumulation: a prev-D agent is in the workgroup total
                # (SUMQ) and not in the prev-C total (SUMQ_C), and SUMQ_D is their difference with
                # their two bounds added.  Its term is > 100 x EACH part's bound, hence > 50 x its own
                # slot's.  (At L = 1000, t = 2 the own-slot ratio is 94 for Q[s0, c]: the median
                # prev-D entry is still an initial draw of ~0.006 while the updated entries of ~0.5
                # make up sum|q|.  Against the parts: 168 and 213.)
                e = k - R.SUMQ_D
                assert med > 100 * max(b[t, R.SUMQ + e], b[t, R.SUMQ_C + e]), (t, R.SLOT_NAMES[k], med)
                assert med > 50 * b[t, k]
                if L > 200:
                    continue
            assert med > 100 * b[t, k], (t, R.SLOT_NAMES[k], med, b[t, k])
        med = _median_term(rec, t, R.SUM_PCT)
        if rec.params.influence_factor == 0.0:
            assert med is None and b[t, R.SUM_PCT] == 0.0
        elif L <= 200:
            assert med > 2 * b[t, R.SUM_PCT], (t, med, b[t, R.SUM_PCT])
        else:
            assert med < 2 * b[t, R.SUM_PCT] and med < 100 * b[t, R.SUM_PCT], (t, med, b[t, R.SUM_PCT])
    assert seen == set(slots)


# ---- 4. the same at late rows ----------------------------------------------------------------------
# Past the eps floor most reputations sit at a bound, few strategies flip, and the prev-D agents whose
# Q sums the kernel forms as total - prev-C are most of the lattice or very few of it (tests/_deep.py).
# The derivations of R.bounds make no assumption about any of that -- the any-order bound is relative
# to sum|x| whatever the terms are, SUMQ_D adds its two parts' bounds whatever their ratio -- so they
# stand as they are; what a late row could break is the margin between the models and the bounds,
# and between the bounds and one agent's term, which is what is held here.  The records are sparse
# (rows = LATE_ROWS): one oracle run of 600 iterations each.
LATE_ROWS = (390, 600)
# (L, operator, M2, replica of its tests/_deep batch); the share of prev-D agents at t = 600: 0.009, 0.82
# (kappa = 0: the NI percent and its bound are exactly 0), 0.11, 0.39, 0.55
LATE_CASES = [(30, "qlearning", True, 2), (30, "qlearning", False, 0), (30, "double_qlearning", True, 1),
              (120, "qlearning", False, 0), (120, "double_qlearning", False, 0)]


@functools.lru_cache(maxsize=None)
def _late(L, alg, M2, k):
    from tests import _deep as D
    b = [b for g in (D.A[3:], D.C, D.D) for b in g if (b.L, b.alg, b.M2, b.state) == (L, alg, M2, "reputation")][0]
    return R.philox_record(L, D.T, b.rows[k], b.seeds[k], k, M2, "reputation", alg, keep_terms=True, rows=LATE_ROWS)


@pytest.mark.parametrize("L,alg,M2,k", LATE_CASES)
def test_late_rows_stay_inside_bounds_and_one_agent_far_outside(L, alg, M2, k):
    rec = _late(L, alg, M2, k)
    assert rec.stop_iter == 0 and rec.rows == LATE_ROWS and rec.rep_dyadic
    assert {t for t, key in rec.terms if key == "grids"} == set(LATE_ROWS)
    p = rec.params
    assert p.reward_weight_rep != 0.0
    for t in LATE_ROWS:
        g = rec.terms[(t, "grids")]
        at_bound = np.mean((g["R"] == p.R_min) | (g["R"] == p.R_max))
        prev_d = np.mean(g["prev_S"] == 1)
        print("L", L, alg, "t", t, "R at a bound %.3f" % at_bound, "prev-D %.3f" % prev_d,
              "flips", int(rec.value[t, R.SW_CD] + rec.value[t, R.SW_DC]))
        assert at_bound > 0.5, (t, at_bound)       # the late lattice, not the early one
    _check_f64(rec, L, LATE_ROWS)
    rng = np.random.RandomState(L + 1)
    _check_finalize(rec, lambda t: model_f64_slots(rec, t, TILES[L], rng)[R.SUM_REW_C], LATE_ROWS)
    _check_pct(rec, L, LATE_ROWS)
    _check_sensitivity(rec, L, LATE_ROWS)
