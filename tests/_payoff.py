"""Shared by the payoff-record tests: a literal per-agent statement of the census row (spgg_abi.h's
words, one agent at a time), the synthetic strategy planes, the rounding bound of the payoff table
against the oracle, the oracle's side of the in-run record, and a NumPy model of the device's pair-sum
scheme (csrc/spgg_payoff.hip: the staged byte K | c << 5 unpacked by masks into the two operands of the
int8 dot, rows padded to dwords, the rotated row window of tests/_reputation.py).  NumPy only."""
import numpy as np

from oracle import spgg_oracle as O
from spgg_amd import payoff as PF
from tests import _params as P
from tests import _reputation as RP

SLOTS, BOND_CD, BOND_CC, BOND_DD = 363, 260, 311, 337     # spgg_abi.h: SPGG_PAYOFF_*
DOT_MAX = 4 * 25 * 25                                     # spgg_pf::kDotMax
LANE_DOTS_MAX = (2 ** 31 - 1) // DOT_MAX                  # spgg_pf::kMaxLaneDots
PAIR_WAVES = 16                                           # spgg_pf::kPairWaves
U = 2.0 ** -53


# ---- the census, one agent at a time ---------------------------------------------------------------------------
def literal_census(S):
    """(row, plane) as spgg_abi.h words them.  Small lattices only."""
    S = np.asarray(S).astype(np.int64) & 1
    L = S.shape[0]
    c = 1 - S
    nb = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))

    def N(y, x):
        return sum(int(c[(y + dy) % L, (x + dx) % L]) for dy, dx in nb)

    def K(y, x):
        return sum(N(y + dy, x + dx) for dy, dx in nb)

    row = [0] * SLOTS
    plane = np.zeros((L, L), dtype=np.uint8)
    for y in range(L):
        for x in range(L):
            sg, k = int(S[y, x]), K(y, x)
            m = N(y, x) - int(c[y, x])
            row[(sg * 5 + m) * 26 + k] += 1
            plane[y, x] = (k | sg << 5 | m << 6) & 0xff
            for y2, x2 in ((y, (x + 1) % L), ((y + 1) % L, x)):
                s2, k2 = int(S[y2, x2]), K(y2, x2)
                if sg != s2:
                    row[BOND_CD + 25 + ((k - k2) if sg == 0 else (k2 - k))] += 1
                else:
                    row[(BOND_CC if sg == 0 else BOND_DD) + abs(k - k2)] += 1
    return np.array(row, dtype=np.int64), plane


# ---- synthetic planes ------------------------------------------------------------------------------------------------
DENSITIES = (0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 0.95)
PATTERN_NAMES = ("all_c", "all_d", "checkerboard", "stripes_1", "stripes_2", "single_d", "single_c") + tuple(
    f"density_{d}" for d in DENSITIES)


def patterns(L, seed=0):
    """{name: (L, L) int64 strategies, 0 = C} in PATTERN_NAMES' order."""
    rs = np.random.RandomState(3000 + 11 * L + seed)
    y, x = np.mgrid[0:L, 0:L]
    one_d, one_c = np.zeros((L, L), dtype=np.int64), np.ones((L, L), dtype=np.int64)
    one_d[L // 3, (2 * L) // 3] = 1
    one_c[(2 * L) // 3, L // 3] = 0
    out = [np.zeros((L, L), dtype=np.int64), np.ones((L, L), dtype=np.int64), (x + y) & 1, x & 1, (y >> 1) & 1, one_d, one_c]
    out += [(rs.rand(L, L) < d).astype(np.int64) for d in DENSITIES]
    return dict(zip(PATTERN_NAMES, out))


def dirty(S, seed):
    """The uint8 plane of strategies S with random bookkeeping bits 1-4 on every byte."""
    rs = np.random.RandomState(seed)
    return (np.asarray(S).astype(np.uint8) & 1) | (rs.randint(0, 16, np.shape(S)) << 1).astype(np.uint8)


# ---- the payoff table against the oracle: the bound ----------------------------------------------------------------
# Both expressions divide by the same double den = fl(4 r - fl(r - 5)) after subtracting the same
# nm = fl(r - 5), and both start from the same A = fl(r c); only the numerators differ.  Against the
# exact E = A K / 5 - 5 cost c_i - nm, with M' = |A| K / 5 + 5 |cost| and M = M' + |nm| (every partial
# result of either expression is at most M in magnitude, up to factors 1 + O(u)):
#   oracle.payoff: per group A * N_g (1 rounding) and / 5 (1): 2 u |A| N_g / 5, over the five groups
#     2 u |A| K / 5; a cooperator's - cost (1 each, on at most |A| N_g / 5 + |cost|): u M' in all; the
#     products with S0 / S1 and the sum of the two are exact (one factor is 0); the sum of the five
#     groups (4, each on a partial sum of at most M'): 4 u M'; - nm (1, on at most M): u M.   <= 8 u M
#   payoff_values: A * K (1) and / 5 (1): 2 u |A| K / 5; 5 * cost (1): u 5 |cost|; the product with
#     c_i is exact; the subtraction (1, on at most M'): u M'; - nm (1): u M.                   <= 5 u M
#   the two divisions round once each, on quotients of at most M / |den|:                        2 u M / |den|
# so |payoff_values - oracle.payoff| <= 15 u M / |den| to first order; 16 covers the second-order terms
# (each factor 1 + delta compounds at most 8 deep: 15 * (1 + 8 u) < 16).  The figure measured over the
# lattices of tests/test_payoff_cpu.py is 2.9 u M / |den| (3.2 u relative to the payoff itself).
VALUE_BOUND_ROUNDINGS = 16


def value_bound(p, K):
    """The bound above for the parameters p (r, c, cost) at the totals K."""
    A, nm = abs(p.r * p.c), abs(p.r - 5)
    den = abs(4 * p.r - (p.r - 5))
    return VALUE_BOUND_ROUNDINGS * U * (A * np.asarray(K, dtype=np.float64) / 5 + 5 * abs(p.cost) + nm) / den


# Sum over the census of count * P(sigma, K) against the oracle's np.sum(P): each of the n terms of either
# sum carries its value's error (value_bound at most, the census side's product count * P one rounding more
# per slot, on a magnitude of count * |P|), and each sum adds at most n - 1 roundings (np.sum's pairwise
# order adds fewer; 52 slots the census side) on partial sums of at most sum |P_i| =: Sabs.  So
#   |sum census * P - sum oracle P| <= sum_i value_bound_i + u Sabs + (n - 1 + 52) u Sabs.
def sum_bound(p, Kfield, Pabs_sum):
    n = np.asarray(Kfield).size
    return float(np.sum(value_bound(p, Kfield)) + (n + 52) * U * Pabs_sum)


CHECK_ROWS = ((2.0, 1.0, 0.5), (3.7, 1.3, 0.2), (5.0, 1.0, 0.5), (0.25, 0.7, 4.0))     # (r, c, cost)
CHECK_SIDES = (3, 4, 5, 13, 18, 37)
CHECK_DENSITIES = tuple(np.linspace(0.05, 0.95, 9))


def oracle_rows():
    """oracle.Params of the check rows and of the rows of tests/_params.EDGE whose normalisation's
    denominator 4 r - (r - 5) is not zero."""
    rows = [O.Params(r=r, c=c, cost=cost) for r, c, cost in CHECK_ROWS]
    for row in P.EDGE.values():
        if 4 * row["r"] - (row["r"] - 5) != 0:
            rows.append(O.Params(r=row["r"], c=row["c"], cost=row["cost"]))
    return rows


# ---- the oracle's side of the in-run record ---------------------------------------------------------------------------
def datasets(e, every, max_d, t0=1):
    """What payoff_histories() gives for a tests/_observers.Trajectory: the host models on the oracle's S_t."""
    its = np.arange(t0, e.last + 1, every, dtype=np.int64)
    rows = np.array([PF.host_payoff_census(e.S[int(t)])[0] for t in its], dtype=np.int64).reshape(len(its), SLOTS)
    d = dict(payoff_history_iters=its, payoff_census_history=rows[:, :BOND_CD].reshape(len(its), 2, 5, 26),
             payoff_bond_history=rows[:, BOND_CD:], payoff_values=PF.payoff_values(e.row))
    if max_d is not None:
        d["payoff_pair_sums_history"] = np.array([PF.host_payoff_pairs(e.S[int(t)], max_d) for t in its],
                                                 dtype=np.int64).reshape(len(its), 2 + 6 * (max_d + 1))
    return d


def compare(got, want, k=0):
    assert list(got) == list(want), (k, list(got), list(want))
    for name, w in want.items():
        g = np.asarray(got[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, name, g.dtype, g.shape, w.dtype, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0]
            raise AssertionError((f"replica {k}", name, "rows", bad[:8].tolist(), g[bad[0]].ravel().tolist(),
                                  w[bad[0]].ravel().tolist()))


# ---- NumPy model of the device's pair-sum scheme -------------------------------------------------------------------------
def staged(plane):
    """uint32 (L, W): the plane's bytes as the kernel stages them, K | c << 5 (bit 5 flipped, the m bits
    dropped), four cells to a dword, the bytes beyond a row's L cells zero."""
    b = ((np.asarray(plane, dtype=np.uint8) ^ 0x20) & 0x3f).astype(np.uint8)
    L, W = b.shape[0], RP.row_dwords(b.shape[0])
    out = np.zeros((L, W * RP.CELLS), dtype=np.uint8)
    out[:, :L] = b
    return out.view("<u4").reshape(L, W)


def k_of(q):
    return np.asarray(q, dtype=np.uint32) & np.uint32(0x1f1f1f1f)


def c_of(q):
    return (np.asarray(q, dtype=np.uint32) >> np.uint32(5)) & np.uint32(0x01010101)


def model_rotate(plane, d):
    """(K, c) (L, L) of the cells the rotated row window pairs with every cell: np.roll(., -d, axis=1)."""
    L = np.asarray(plane).shape[0]
    rot = RP.rotated_dwords(staged(plane), d, L)
    cells = lambda q: np.ascontiguousarray(q.astype("<u4")).view(np.uint8).reshape(L, -1)[:, :L].astype(np.int64)   # noqa: E731
    return cells(k_of(rot)), cells(c_of(rot))


def model_pairs(plane, max_d):
    """The pair-sum row the way the LDS instances compute it: four dots per dword pair on the unpacked
    operands (the rotated dword's bytes beyond the row meet zero padding), lane partials of a 64-lane
    wave held to int32, reduced in int64."""
    L = np.asarray(plane).shape[0]
    W = RP.row_dwords(L)
    lat = staged(plane)
    flat = lat.reshape(-1)
    lanes = np.arange(flat.size) % 64

    def dot(a, b):
        out = RP.dot4(a, b)
        assert np.all(out >= 0) and np.all(out <= DOT_MAX)
        return out

    def reduce(dots):
        part = np.zeros(64, dtype=np.int64)
        np.add.at(part, lanes, dots)
        assert np.all(part < 2 ** 31)
        return int(part.sum())

    def triple(own, v):
        return (reduce(dot(k_of(own), k_of(v))), reduce(dot(c_of(own), k_of(v)) + dot(k_of(own), c_of(v))),
                reduce(dot(c_of(own), c_of(v))))

    ones = np.full(flat.size, 0x01010101, dtype=np.uint32)
    out = np.zeros(2 + 6 * (max_d + 1), dtype=np.int64)
    out[0], out[1] = reduce(dot(k_of(flat), ones)), reduce(dot(c_of(flat), ones))
    tri = out[2:].reshape(2, max_d + 1, 3)
    for d in range(max_d + 1):
        tri[0, d] = triple(flat, RP.rotated_dwords(lat, d, L).reshape(-1))
        tri[1, d] = triple(flat, flat[(np.arange(flat.size) + d * W) % flat.size])
    return out


def lane_dots_global(L):
    """spgg_pf::lane_dots_global: dword pairs one lane of the global instance adds up."""
    return ((L + PAIR_WAVES - 1) // PAIR_WAVES) * ((RP.row_dwords(L) + 63) // 64)


def max_side():
    """The static_asserts' formula for spgg_payoff_pairs_max_side: the largest L with L * L < 2^31 whose
    lane partials fit int32."""
    L = int(np.sqrt(2.0 ** 31)) + 2
    while L * L >= 2 ** 31 or lane_dots_global(L) > LANE_DOTS_MAX:
        L -= 1
    return L
