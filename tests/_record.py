"""The device history record stats[t][SPGG_NSTAT] of one replica, EXACTLY, and per-slot error bounds.

exact_record() runs the oracle and sums its per-agent arrays with math.fsum (the correctly rounded
exact sum) at the slot indices include/spgg_abi.h documents; bounds() says how far the device may
be from that: 0 (bit-equal) or an absolute bound derived from the operations the step kernel and
spgg_history_finalize_kernel execute (csrc/spgg_kernels.hip).  No bound is fitted to what the
device returns.  NumPy + math only; independent of engine.histories_from_stats.

Notation: u = 2^-53 (f64 unit roundoff), v = 2^-24 (f32), n = L * L agents.  A "rounding" is one
floating-point operation, relative error <= u of its result.  Every bound is first order in u
(v); the second-order terms are below (n u)^2 < 2^-60 of the first at n = 10^6 and are covered by
the factor SECOND_ORDER = 1 + 2^-20 on every bound.
"""
import dataclasses
import math

import numpy as np

from oracle import philox as PH
from oracle import spgg_oracle as O

NSTAT = 34
NCOOP, SUMP, SUMP_C, SUMP_D, SUMR, SW_CD, SW_DC, SUM_WPP, SUM_WRR = range(9)
SUM_REW_C, SUM_REW_D, SUM_RATIO_C, GC0 = 9, 10, 11, 12
NMD_POS, NMD_POS2, SUM_PCT, SUMQ, SUMQ_C, SUMQ_D, GMAX = 18, 19, 20, 21, 25, 29, 33
SLOT_NAMES = (["NCOOP", "SUMP", "SUMP_C", "SUMP_D", "SUMR", "SW_CD", "SW_DC", "SUM_WPP", "SUM_WRR",
               "SUM_REW_C", "SUM_REW_D", "SUM_RATIO_C"] + [f"GC{d}" for d in range(6)]
              + ["NMD_POS", "NMD_POS2", "SUM_PCT"] + [f"{g}{e}" for g in ("SUMQ", "SUMQ_C", "SUMQ_D") for e in range(4)]
              + ["GMAX"])
assert len(SLOT_NAMES) == NSTAT

U = 2.0 ** -53
V = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126
SECOND_ORDER = 1.0 + 2.0 ** -20

COUNTERS = (NCOOP, SW_CD, SW_DC, NMD_POS, NMD_POS2) + tuple(range(GC0, GC0 + 6))
# slots the step kernel fills when launch t+1 (or the flush) finalises iteration t: phase 1a
PENDING_SLOTS = (SUM_PCT,) + tuple(range(SUMQ, SUMQ + 12))
# f64 float slots whose per-agent terms a sum can lose or repeat (sensitivity tests)
F64_SUM_SLOTS = (SUMR, SUM_REW_C, SUM_RATIO_C) + tuple(range(SUMQ, SUMQ + 12))
REGROUPED = (SUMP, SUMP_C, SUMP_D, SUM_WPP, SUM_REW_D)

# The runner's parameters the GPU record tests vary (tests/test_gpu_record.py), and the lattices
# they run: L -> (tile width, tile height, agents per thread, history stripes) of a model of the
# device's summation order (tests/test_record_bounds_cpu.py; the bounds hold for any order, so the
# model tiles need not be the library's, only of its kind: tiles that do not divide L, invalid
# slots, several stripes at L = 1000).  L = 200 is there for the f32 slot's limit.
BASE = dict(c=1, cost=1, alpha=0.8, gamma=0.9, epsilon=0.5, epsilon_decay=0.99, epsilon_min=0.01,
            lambda_epsilon=0.01, delta_R_D=1, R_min=-10, R_max=10, rep_gain_C=1.0, reward_weight_payoff=0.95,
            influence_factor=1.0, r=3.0)
GPU_LATTICES = {12: (12, 12, 1, 1), 13: (13, 13, 1, 1), 16: (16, 16, 1, 1), 18: (18, 18, 4, 1), 24: (24, 10, 1, 1),
                30: (30, 8, 1, 1), 60: (20, 25, 2, 1), 80: (27, 27, 4, 1), 120: (40, 24, 4, 1),
                1000: (40, 25, 4, 16)}

PARAM_KEYS = ("r", "c", "cost", "alpha", "gamma", "epsilon", "epsilon_decay", "epsilon_min", "influence_factor",
              "lambda_epsilon", "delta_R_D", "R_min", "R_max", "reward_weight_payoff", "rep_gain_C")


@dataclasses.dataclass
class Record:
    value: np.ndarray          # (T+2, NSTAT) the exact sums, correctly rounded (counters / GMAX: exact)
    mag: np.ndarray            # (T+2, NSTAT) sum |term| of the accumulated slots
    pay_mag: np.ndarray        # (T+2,) "mag" of the regrouped payoff slots of iteration t (see bounds)
    last: int                  # iterations with a start record (the absorbing one included)
    stop_iter: int             # 0, or the absorbing iteration (== last)
    n: int
    params: O.Params
    rep_dyadic: bool           # this replica's reputations are multiples of a dyadic unit (int8 path)
    rep_units_max: float       # max over t of sum |R_t / unit| (the int8 path's integer sum), else 0
    final: dict                # the oracle's final state
    terms: dict                # (t, k) -> per-agent terms of the float slots (keep_terms), else {}
    rows: tuple = None         # the iterations whose accumulated float slots were evaluated (None: all)


def oracle_params(params, L, T, M2, state, algorithm):
    """O.Params from an O.Params, a dict of PARAM_KEYS or an object with those attributes; the
    operator's own alg_alpha / alg_gamma are carried over where the dict or object has them."""
    over = dict(L=L, iterations=T, use_second_order=M2, state_representation=state, algorithm=algorithm)
    if isinstance(params, O.Params):
        return dataclasses.replace(params, **over)
    keys = PARAM_KEYS + ("alg_alpha", "alg_gamma")
    kw = dict(params) if isinstance(params, dict) else {k: getattr(params, k) for k in keys if hasattr(params, k)}
    return O.Params(**{k: v for k, v in kw.items() if k in keys}, **over)


def _rep_unit(p):
    """The dyadic unit of engine.ReplicaParams.rep_unit (restated: this module imports no engine)."""
    vals = [float(p.rep_gain_C), float(p.delta_R_D), float(p.R_min), float(p.R_max)]
    if vals[2] > vals[3] or vals[2] > 0 or vals[3] < 0:
        return None
    for m in range(11):
        ks = [x * 2.0 ** m for x in vals]
        if all(k == int(k) for k in ks):
            g, l_, lo, hi = (int(k) for k in ks)
            return 2.0 ** -m if -128 <= lo and hi <= 127 and abs(g) <= 127 and abs(l_) <= 127 else None
    return None


def _fsum(x):
    return math.fsum(np.asarray(x, dtype=np.float64).ravel().tolist())


def exact_record(params, L, T, M2, state, algorithm, rs=None, draws=None, init=None, keep_terms=False, rows=None):
    """The exact history record of one replica.

    rs: the RandomState of a RandomState run (init None: it also makes SPGG.__init__'s draws, as
    engine.reference_init does); draws: i -> draw dict of a counter-based run (oracle/philox.py);
    init: an object with Q, S and (Double-Q) tables replacing the initial draws.

    rows: the iterations at which the accumulated float slots -- all that goes through put(), and
    pay_mag -- are evaluated (math.fsum is most of a record's cost: a long run pays it on the
    rows it looks at); the other rows keep 0 there.  The counters, the group composition and GMAX
    are filled on every row whatever `rows` is, and keep_terms keeps the terms of those rows only.
    None: every row."""
    rows = None if rows is None else tuple(sorted({int(t) for t in rows}))
    on_row = (lambda t: True) if rows is None else frozenset(rows).__contains__
    p = oracle_params(params, L, T, M2, state, algorithm)
    n = L * L
    if init is None:
        Q0, tables0 = O.init_tables(p, rs)
        S0 = rs.randint(0, 2, size=(L, L))
    else:
        Q0, tables0, S0 = init.Q, init.tables, np.asarray(init.S)
    val = np.zeros((T + 2, NSTAT))
    mag = np.zeros((T + 2, NSTAT))
    pay_mag = np.zeros(T + 2)
    terms = {}
    unit = _rep_unit(p)
    w_p, w_rep = p.reward_weight_payoff, p.reward_weight_rep
    state_ = dict(R=np.zeros((L, L)), units=0.0)
    rc = p.r * p.c
    pay_c = np.array([rc * N / 5 - p.cost for N in range(6)])     # spgg.py:256-257, as ReplicaParams.to_c
    pay_d = np.array([rc * N / 5 for N in range(6)])
    norm_den = 4 * p.r - (p.r - 5)

    def put(t, k, x):
        if not on_row(t):
            return
        x = np.asarray(x, dtype=np.float64).ravel()
        val[t, k] = _fsum(x)
        mag[t, k] = _fsum(np.abs(x))
        if keep_terms:
            terms[(t, k)] = x.copy()

    def group_comp(t, S):      # composition of the groups of S -> slot t, and the regrouped slots' mag of t+1
        nd = O.sum5((S == 1).astype(int))
        gc = np.array([np.sum(nd == d) for d in range(6)], dtype=np.float64)
        val[t, GC0:GC0 + 6] = gc
        raw = sum(gc[d] * ((5 - d) * abs(pay_c[5 - d]) + d * abs(pay_d[5 - d])) for d in range(6))
        if on_row(t + 1):
            pay_mag[t + 1] = (raw + n * abs(p.r - 5)) / abs(norm_den)

    def start(t, S, R, P):     # iteration-start values of t (spgg.py:380-394)
        val[t, NCOOP] = np.sum(S == 0)
        put(t, SUMP, P)
        put(t, SUMP_C, P[S == 0])
        put(t, SUMP_D, P[S == 1])
        put(t, SUMR, R)
        if unit is not None:
            state_["units"] = max(state_["units"], float(np.sum(np.abs(R / unit))))

    def on_step(i, S_new, R_new, Q, d):
        a, ps, P = d["_actions"], d["_prev_S"], d["_P"]
        if i == 1:
            group_comp(0, ps)
        R_start = state_["R"]
        start(i, ps, R_start, P)
        state_["R"] = R_new
        rew, rr = d["_rewards"], d["_rep_reward"]
        val[i + 1, NCOOP] = np.sum(a == 0)
        val[i, SW_CD] = np.sum((ps == 0) & (a == 1))
        val[i, SW_DC] = np.sum((ps == 1) & (a == 0))
        put(i, SUM_WPP, w_p * P)                                   # spgg.py:425
        put(i, SUM_WRR, w_rep * rr)                                # spgg.py:426
        put(i, SUM_REW_C, rew[a == 0])                             # spgg.py:542
        put(i, SUM_REW_D, rew[a == 1])                             # spgg.py:543
        wr = w_rep * rr
        put(i, SUM_RATIO_C, ((np.abs(wr) / (np.abs(rew) + 1e-9)) * 100)[a == 0])   # spgg.py:533-535
        group_comp(i, a)
        md, mi, nu = d["_max_diff"], d["_max_idx"], d["_nu"]
        val[i, NMD_POS] = np.sum(md > 0)
        val[i, NMD_POS2] = np.sum((md > 0) & (mi >= 4))
        put(i, SUM_PCT, np.abs(nu) / (d["_atd2"] + np.abs(nu) + 1e-8) * 100)       # spgg.py:512
        val[i, GMAX] = max(0.0, float(np.max(md)))                 # max over the lattice of max(0, max_diff)
        for e in range(4):                                         # spgg.py:561-583 (Double-Q: the mean table)
            qv = Q[:, :, e // 2, e % 2]
            put(i, SUMQ + e, qv)
            put(i, SUMQ_C + e, qv[ps == 0])
            put(i, SUMQ_D + e, qv[ps == 1])
        if keep_terms and on_row(i):
            # the lattice-shaped operands, for a model of the device's summation order
            terms[(i, "grids")] = dict(prev_S=ps.copy(), actions=a.copy(), Q=Q.copy(), rew=rew.copy(), wr=wr.copy(),
                                       nu=nu.copy(), atd2=d["_atd2"].copy(), R=R_start.copy())

    _, fin = O.run(p, rs, S_init=S0, Q_init=Q0, tables_init=tables0, collect_snapshots=False, on_step=on_step,
                   draws=draws)
    stop = int(fin["stop_iter"])
    last = stop if stop else T
    if stop:        # the absorbing iteration: its start record only (spgg.py:380-406)
        if stop == 1:
            group_comp(0, fin["S"])
        start(stop, fin["S"], fin["R"], fin["P"])
    return Record(value=val, mag=mag, pay_mag=pay_mag, last=last, stop_iter=stop, n=n, params=p,
                  rep_dyadic=unit is not None, rep_units_max=state_["units"], final=fin, terms=terms,
                  rows=rows)


def philox_record(L, T, params, seed, stream_id, M2, state, algorithm="qlearning", init=None, keep_terms=False,
                  rows=None):
    """exact_record under the Philox draws of (seed, stream_id), initialised as the engine
    initialises a replica: SPGG.__init__'s draws from RandomState(seed) unless init is given."""
    key = PH.philox_key(int(seed or 0), stream_id)
    rs = None if init is not None else np.random.RandomState(seed)
    return exact_record(params, L, T, M2, state, algorithm, rs=rs, init=init, keep_terms=keep_terms, rows=rows,
                        draws=lambda i: PH.draws(key, L, i, algorithm))


# ---- the bounds --------------------------------------------------------------------------------
# Roundings counted from csrc/spgg_kernels.hip (compiled with -ffp-contract=off: no operation below
# is fused unless written as an FMA) and from the oracle's NumPy expressions.
#
# Any-order summation.  A slot accumulated in f64 is a tree of additions over the n per-agent terms
# in an order the hardware chooses: per thread `v = fma(x, mask, v)` with mask 0 or 1 (x * 1 and
# x * 0 are exact: one rounding, that of x + v), the wave's exchange tree (wave_partials), the four
# wave totals added in the epilogue, one f64 atomicAdd per workgroup onto its stripe, the stripes
# added by stats_folded.  Additions of an exact 0 (masked terms, invalid slots, the zero-initialised
# record) round nothing, so at most n - 1 additions round, and for ANY such tree
#     |computed - exact| <= (n - 1) u sum|x_i|      (Jeannerod & Rump, SIAM J. Matrix Anal. 2013),
# which is what the issue's emulation stays three orders below.  ANY_ORDER(n) = (n - 1) u.
#
# rcp_diag(x): the hardware reciprocal estimate r0 = (1/x)(1 + e0) and two Newton steps
# r <- fma(r, fma(-x, r, 1), r).  A step squares the error and adds its roundings: the residual
# fma(-x, r, 1) is one rounding of a quantity of size e, the update one rounding of r: after two
# steps |e2| <= u + e0^4 + O(u e0^2), below 2u = 1 ulp for any estimate good to e0 <= 2^-14.
K_RCP_DIAG = 2
# SUM_RATIO_C, per term beyond the summation: the oracle rounds |wr| / x and * 100 (2); the kernel
# rounds rcp_diag (K_RCP_DIAG), |wrr| * rcp (1) and the * 100 on each workgroup total (1, relative to
# a partial sum of non-negative terms, so to no more than sum|x_i| in all).  x = |rew| + 1e-9 is the
# same double on both sides (the rewards are bit-exact: they decide the state).
K_RATIO = 2 + K_RCP_DIAG + 1 + 1
# Double-Q: the kernel's mean2(q1, q2) = (q1 + q2) * 0.5 makes the one rounding the oracle's
# (Q1 + Q2) / 2 makes, on the same operands (the tables are bit-exact; halving is exact): the
# per-agent terms are the same doubles.  Likewise Q, R and the rewards of the other operators.
K_MEAN2 = 0
#
# Regrouped payoff slots (spgg_history_finalize_kernel).  With the table values c_N = pay_c[N],
# d_N = pay_d[N] (the same doubles on both sides: ReplicaParams.to_c computes them in the oracle's
# order), the oracle's P_i is a rounded evaluation of ideal_i = (sum of the agent's five group
# payoffs - (r - 5)) / norm_den: four additions, one subtraction, one division, each rounding a
# partial result of size <= mag_i = (sum |group payoffs| + |r - 5|) / |norm_den|: 6 roundings of
# <= u mag_i.  Summed over the lattice, ideal regroups EXACTLY: a group centred on a cell with d
# defectors pays (5 - d) c_{5-d} + d d_{5-d}, so sum_i ideal_i = (sum_d GC_d ((5-d) c_{5-d} + d d_{5-d})
# - n (r - 5)) / norm_den and sum_i mag_i = mag, the issue's magnitude.  math.fsum adds one rounding
# of the total (<= u mag).
K_REF_P = 6 + 1
# The kernel evaluates the regrouped form: per d the coefficient (5-d)*c + d*d (2 products + 1 add:
# 3), gc * coefficient (1), five rounding accumulations of six terms (5): 9 roundings of <= u times
# the sum of the terms' magnitudes; then n * norm_min (1), the subtraction (1), the division (1).
K_DEV_SUMP = 9 + 3
# SUMP_C: coefficient (5-d)*c (1), product (1), accumulations (5), nc * norm_min, -, / (3).
K_DEV_SUMP_C = 7 + 3
K_SUMP = K_REF_P + K_DEV_SUMP                       # 19
K_SUMP_C = K_REF_P + K_DEV_SUMP_C                   # 17
K_SUMP_D = K_REF_P + K_DEV_SUMP + K_DEV_SUMP_C + 1  # sump - sump_c: both parts and the subtraction: 30
# SUM_WPP = w_p * sump: the kernel adds one product; the oracle rounds w_p * P_i per agent (1 more
# than K_REF_P).  Everything scales with |w_p|.
K_WPP = (K_REF_P + 1) + (K_DEV_SUMP + 1)            # 21
# SUM_WRR: the oracle's terms w_rep * 0.5 (or * 0) are exact, so fsum returns the correctly rounded
# real nc1 * (w_rep / 2); the kernel's nc1 * (w_rep * 0.5) is one product of the same two exact
# operands: the same correctly rounded real.  Bit-equal: K = 0.
K_WRR = 0
# SUM_REW_D = (wpp + wrr) - SUM_REW_C.  Oracle: rew_i = fl(fl(w_p P_i) + wr_i): 6 + 1 roundings of
# w_p mag_i and one of (w_p mag_i + wr_i); sum over D = sum over all - sum over C, and fsum rounds
# the total once.  Kernel: wpp (K_DEV_SUMP + 1 of |w_p| mag), wrr (1 of its size W = nc1 |w_rep| / 2),
# the addition (1 of |w_p| mag + W), the subtraction (1 of |w_p| mag + W + sum|rew_C| <= 2 (|w_p| mag + W)),
# plus whatever SUM_REW_C itself is off by (its any-order bound).
K_REWD_P = (6 + 1 + 1) + (K_DEV_SUMP + 1) + 1 + 2 + 1   # on |w_p| mag: 25
K_REWD_W = 1 + 1 + 1 + 2 + 1                            # on W: 6
#
# SUM_PCT, the one f32 chain (phase 1a): term = anu * rcpf((atdv + anu) + 1e-8f), accumulated per
# thread with fmaf over its <= apt_max agents, then (double) and the f64 reduction, * 100 per
# workgroup.  In units of v = 2^-24 relative to the term (every term is in [0, 1] and nothing
# cancels: errors of the denominator are relative to it too):
#   (float)nu                     1   numerator
#   (float)|alpha td'|, (float)nu 1   denominator, jointly (v * (atd + anu) <= v * den)
#   the two f32 additions         2
#   1e-8f for 1e-8                1   (|1e-8f - 1e-8| <= v * 1e-8 <= v * den)
#   v_rcp_f32                     2   1 ulp, the accuracy the ISA documents = 2 v
#   anu * rcp                     1
#   fmaf accumulations            apt_max - 1 + 1   (the first adds to an exact 0; one spare for the
#                                 issue's count of apt_max)
# = 8 + apt_max (12 at four agents per thread).  The f64 side -- the oracle's two additions, its
# division and * 100, the kernel's * 100 and the any-order sum -- adds (5 + n - 1) u.
def k32(apt_max):
    return 8 + apt_max
# Flush to zero: v_rcp_f32 and the casts may flush f32 subnormals.  |nu| < 2^-126 flushed: the true
# term is below 2^-126 / 1e-8; |alpha td'| flushed: the denominator (>= 1e-8) moves by 2^-126, the
# term (<= 1) by 2^-126 / 1e-8 relatively; the product underflowing: 2^-126.  Per agent, times the
# 100, times n.
PCT_FLUSH_PER_AGENT = 100.0 * F32_MIN_NORMAL * (2e8 + 1)


def any_order(n):
    return (n - 1) * U


def bounds(rec, n=None, apt_max=4, rep_int8=None):
    """(T+2, NSTAT) absolute bounds on |device - rec.value|; 0.0 = the slot is bit-equal.

    rep_int8: whether the batch runs the int8 reputation path (every replica dyadic; default:
    this replica's own)."""
    n = rec.n if n is None else n
    p = rec.params
    if rep_int8 is None:
        rep_int8 = rec.rep_dyadic
    T2 = rec.value.shape[0]
    b = np.zeros((T2, NSTAT))      # counters, GMAX (an order-free max of bit-exact differences), SUM_WRR,
                                   # and every slot nothing is added to (past `last`, the step slots of an
                                   # absorbing iteration, slot 0 but its group composition): exact
    ao = any_order(n)
    w_p, w_rep = abs(p.reward_weight_payoff), abs(p.reward_weight_rep)
    mag = rec.mag
    # f64 accumulated slots: per-agent terms equal to the oracle's (K_MEAN2 = 0 extra roundings)
    for k in (SUM_REW_C,) + tuple(range(SUMQ, SUMQ + 4)) + tuple(range(SUMQ_C, SUMQ_C + 4)):
        b[:, k] = (ao + K_MEAN2 * U) * mag[:, k]
    # SUMR: int8 path -- an integer sum of R / unit times the dyadic unit, exact while it stays below
    # 2^53 (rep_units_max; test_record_bounds_cpu.py); f64 path -- any order
    if rep_int8:
        assert rec.rep_dyadic and rec.rep_units_max < 2.0 ** 53
    else:
        b[:, SUMR] = ao * mag[:, SUMR]
    # SUM_RATIO_C: exactly 0 when w_rep == 0 (the kernel skips it; the oracle's terms are 0 / x)
    if w_rep != 0.0:
        b[:, SUM_RATIO_C] = (ao + K_RATIO * U) * mag[:, SUM_RATIO_C]
    # sums over prev-D: each workgroup's total minus its prev-C total (epilogue: tot0 - tot1), then the
    # atomics.  A workgroup of m agents rounds m - 1 additions in each part and one subtraction, the W
    # workgroups' differences W - 1 additions more, each relative to no more than the parts'
    # magnitudes: (m - 1 + 1 + W - 1) u <= (m W - 1) u = (n - 1) u on (sum|q| + sum|q_C|): the two
    # parts' bounds added.
    for e in range(4):
        b[:, SUMQ_D + e] = b[:, SUMQ + e] + b[:, SUMQ_C + e]
    # regrouped payoff slots: K u mag, independent of n
    pm = rec.pay_mag
    b[:, SUMP] = K_SUMP * U * pm
    b[:, SUMP_C] = K_SUMP_C * U * pm
    b[:, SUMP_D] = K_SUMP_D * U * pm
    b[:, SUM_WPP] = K_WPP * U * w_p * pm
    b[:, SUM_WRR] = K_WRR * U * mag[:, SUM_WRR]
    wsize = np.zeros(T2)
    wsize[:-1] = rec.value[1:, NCOOP] * (w_rep * 0.5)          # W of step t: C actions = NCOOP of slot t + 1
    b[:, SUM_REW_D] = U * (K_REWD_P * w_p * pm + K_REWD_W * wsize) + b[:, SUM_REW_C]
    # the f32 NI percent: exactly 0 when kappa == 0 (nu = +0; the kernel skips the term)
    if p.influence_factor != 0.0:
        b[:, SUM_PCT] = (k32(apt_max) * V + (5 + n - 1) * U) * mag[:, SUM_PCT] + n * PCT_FLUSH_PER_AGENT
    b *= SECOND_ORDER
    # nothing is accumulated outside the executed iterations: start values up to `last`, step values
    # up to m (the absorbing iteration records its start only), NCOOP one slot further
    m = rec.last - 1 if rec.stop_iter else rec.last
    step_slots = [k for k in range(NSTAT) if k not in (NCOOP, SUMP, SUMP_C, SUMP_D, SUMR)]
    b[0, :] = 0.0
    b[rec.last + 1:, :] = 0.0
    b[m + 1:, step_slots] = 0.0
    return b


def mismatches(got, rec, bound, rows=None, skip=()):
    """[(t, slot name, got, want, bound)] of the slots of `got` (T+2, NSTAT) outside the bounds;
    rows: the slots t to look at (default all); skip: slot indices left out."""
    bad = []
    want = rec.value
    ts = range(want.shape[0]) if rows is None else rows
    for t in ts:
        for k in range(NSTAT):
            if k in skip:
                continue
            g, w, bd = float(got[t, k]), float(want[t, k]), float(bound[t, k])
            if not abs(g - w) <= bd:        # (a NaN fails)
                bad.append((t, SLOT_NAMES[k], g, w, bd))
    return bad


def mismatches_on_rows(got, rec, bound):
    """mismatches() for a record made with `rows`: the counters and GMAX, which exact_record fills
    on every row, on every row (their bound is 0: bit-equal); the other slots where the record
    holds them -- on rec.rows, and past rec.last, where nothing is accumulated and every slot of
    the record is 0 whatever `rows` was.  rec.rows None: mismatches(got, rec, bound)."""
    if rec.rows is None:
        return mismatches(got, rec, bound)
    every = COUNTERS + (GMAX,)
    assert not bound[:, list(every)].any()
    T2 = rec.value.shape[0]
    held = sorted({t for t in rec.rows if 0 <= t < T2} | set(range(rec.last + 1, T2)))
    bad = mismatches(got, rec, bound, skip=[k for k in range(NSTAT) if k not in every])
    return sorted(bad + mismatches(got, rec, bound, rows=held, skip=every), key=lambda m: m[0])
