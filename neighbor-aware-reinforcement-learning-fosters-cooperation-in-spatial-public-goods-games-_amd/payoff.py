"""The payoff field's record: how payoffs are distributed among cooperators and among defectors, who
earns more across a C-D interface, and over what distance payoffs are correlated (spgg_payoff_census,
spgg_payoff_pairs, spgg_abi.h).

With c = 1 on cooperators (bit 0 of S_t clear), sum5 the 5-point periodic sum, N = sum5(c) and
K = sum5(N) in 0 .. 25, an agent's five group counts are N at its own cell and at its four neighbours,
so in real arithmetic its normalised payoff is

    P = ((r c / 5) K - 5 cost c_i - (r - 5)) / (4 r - (r - 5))

and (sigma, K), sigma = 1 - c, determines it: the integer census of (sigma, K) is the payoff
distribution, for any parameters.  One census row holds census[sigma][m][K] (m = N - c, the agent's
cooperating von-Neumann neighbours), and the bonds between right / lower neighbours by their difference
in K: bond_cd[K_C - K_D + 25], bond_cc[|dK|], bond_dd[|dK|].  The pair sums of K and c at the distances
0 .. D along rows and columns give the two-point function of the payoff.

`host_payoff_census` / `host_payoff_pairs` are the NumPy models (np.roll, nothing of the device's
scheme); `Payoff` the in-run record (the kind "payoff" of records.KINDS).
"""
from __future__ import annotations

import numpy as np

from . import _lib as C
from .records import Record, _every, asis, count, register, specs

PAYOFF_SLOTS = C.PAYOFF_SLOTS
MAX_K = 25
CENSUS_SHAPE = (2, 5, MAX_K + 1)

PAYOFF_DATASETS = ("payoff_history_iters", "payoff_census_history", "payoff_bond_history", "payoff_values")
PAYOFF_PAIRS_DATASET = "payoff_pair_sums_history"
PAYOFF_MAP_DATASET = "payoff_map_final"


def pairs_width(max_d: int) -> int:
    """int64 values of one pair-sum row: sum K, sum c, then (KK, CK, CC) for d = 0 .. max_d along rows,
    then along columns."""
    return 2 + 6 * (int(max_d) + 1)


def _sum5(A):
    return A + np.roll(A, -1, axis=0) + np.roll(A, 1, axis=0) + np.roll(A, -1, axis=1) + np.roll(A, 1, axis=1)


def payoff_fields(S):
    """(sigma, m, K) int64 (L, L) of one lattice: the strategy (bit 0 of S), the cooperating
    von-Neumann neighbours and the group-cooperator total."""
    sigma = np.asarray(S).astype(np.int64) & 1
    if sigma.ndim != 2 or sigma.shape[0] != sigma.shape[1]:
        raise ValueError(f"a square lattice, got {sigma.shape}")
    c = 1 - sigma
    N = _sum5(c)
    return sigma, N - c, _sum5(N)


def plane_byte(sigma, m, K):
    """The plane's byte: K in bits 0-4, sigma in bit 5, the low two bits of m in bits 6-7."""
    return ((K | sigma << 5 | m << 6) & 0xff).astype(np.uint8)


def host_payoff_census(S):
    """(row, plane) of one lattice on the host: the int64 row of PAYOFF_SLOTS counts and the uint8
    plane.  What spgg_payoff_census gives on the device."""
    sigma, m, K = payoff_fields(S)
    row = np.zeros(PAYOFF_SLOTS, dtype=np.int64)
    row[:C.PAYOFF_BOND_CD] = np.bincount(((sigma * 5 + m) * (MAX_K + 1) + K).ravel(), minlength=C.PAYOFF_BOND_CD)
    for axis in (1, 0):                                   # the right and the lower neighbour
        s2, K2 = np.roll(sigma, -1, axis=axis), np.roll(K, -1, axis=axis)
        cd = sigma != s2
        dK = np.where(sigma == 0, K - K2, K2 - K)         # K_C - K_D
        row[C.PAYOFF_BOND_CD:C.PAYOFF_BOND_CC] += np.bincount(dK[cd] + MAX_K, minlength=2 * MAX_K + 1)
        for sg, base in ((0, C.PAYOFF_BOND_CC), (1, C.PAYOFF_BOND_DD)):
            like = ~cd & (sigma == sg)
            row[base:base + MAX_K + 1] += np.bincount(np.abs(K - K2)[like], minlength=MAX_K + 1)
    return row, plane_byte(sigma, m, K)


def host_payoff_pairs(S, max_d=None):
    """The int64 pair-sum row of one lattice on the host, D = max_d (None: L // 2): [sum K, sum c], then
    for d = 0 .. D along rows (roll(., -d, axis=1)), then along columns (axis=0), the triple
    KK[d] = sum K K', CK[d] = sum (c K' + K c'), CC[d] = sum c c'.  What spgg_payoff_pairs gives."""
    sigma, _, K = payoff_fields(S)
    c = 1 - sigma
    L = K.shape[0]
    D = L // 2 if max_d is None else int(max_d)
    if D < 0 or D > L // 2:
        raise ValueError(f"host_payoff_pairs: 0 <= max_d <= L // 2, got {max_d}")
    out = np.empty(pairs_width(D), dtype=np.int64)
    out[0], out[1] = K.sum(), c.sum()
    tri = out[2:].reshape(2, D + 1, 3)
    for a, axis in enumerate((1, 0)):
        for d in range(D + 1):
            K2, c2 = np.roll(K, -d, axis=axis), np.roll(c, -d, axis=axis)
            tri[a, d] = (K * K2).sum(), (c * K2 + K * c2).sum(), (c * c2).sum()
    return out


def split_census(row):
    """(census (.., 2, 5, 26), bond_cd (.., 51), bond_cc (.., 26), bond_dd (.., 26)) views of census rows."""
    row = np.asarray(row)
    return (row[..., :C.PAYOFF_BOND_CD].reshape(row.shape[:-1] + CENSUS_SHAPE), row[..., C.PAYOFF_BOND_CD:C.PAYOFF_BOND_CC],
            row[..., C.PAYOFF_BOND_CC:C.PAYOFF_BOND_DD], row[..., C.PAYOFF_BOND_DD:PAYOFF_SLOTS])


def split_pairs(row, max_d):
    """(sum K, sum c, rows (.., D + 1, 3), cols (.., D + 1, 3)) of pair-sum rows; the last axis: KK, CK, CC."""
    row = np.asarray(row)
    tri = row[..., 2:].reshape(row.shape[:-1] + (2, int(max_d) + 1, 3))
    return row[..., 0], row[..., 1], tri[..., 0, :, :], tri[..., 1, :, :]


def _rcc(params):
    get = params.get if isinstance(params, dict) else lambda k: getattr(params, k)
    return get("r"), get("c"), get("cost")


def payoff_values(params) -> np.ndarray:
    """f64 (2, 26): the normalised payoff P(sigma, K) of an agent of strategy sigma whose five groups
    hold K cooperators in all, for the parameters' r, c, cost (an object or a dict)."""
    r, c, cost = _rcc(params)
    K = np.arange(MAX_K + 1)
    ci = np.array([[1], [0]])
    return (r * c * K / 5 - 5 * cost * ci - (r - 5)) / (4 * r - (r - 5))


def payoff_distribution(census, params, strategy=None):
    """(values ascending, counts int64) of the payoffs a census row (or its (2, 5, 26) census) holds:
    of everybody, or of strategy 0 (C) / 1 (D) alone.  Empty slots are left out."""
    census = np.asarray(census)
    if census.shape[-1] == PAYOFF_SLOTS:
        census = split_census(census)[0]
    if census.shape != CENSUS_SHAPE:
        raise ValueError(f"payoff_distribution: one census row or its {CENSUS_SHAPE} census, got {census.shape}")
    counts = census.sum(axis=1).astype(np.int64)           # (sigma, K)
    P = payoff_values(params)
    if strategy is not None:
        counts, P = counts[int(strategy)], P[int(strategy)]
    counts, P = counts.ravel(), P.ravel()
    order = np.argsort(P[counts > 0], kind="stable")
    return P[counts > 0][order], counts[counts > 0][order]


def gini(values, counts) -> float:
    """Gini coefficient of a weighted distribution: the mean absolute difference over twice the mean;
    nan for an empty distribution or a zero mean."""
    x, w = np.asarray(values, dtype=np.float64), np.asarray(counts, dtype=np.float64)
    W = w.sum()
    mean = (x * w).sum() / W if W else 0.0
    if not W or mean == 0:
        return float("nan")
    mad = (np.abs(x[:, None] - x[None, :]) * w[:, None] * w[None, :]).sum() / (W * W)
    return float(mad / (2 * mean))


TIE_ULPS = 8     # interface_advantage: r c dK and 25 cost are equal within this many units in the last place


def interface_advantage(row, params):
    """(more, same, less): the shares of the C-D bonds of a census row on which the cooperator's payoff
    is above / equal to / below the defector's: r c (K_C - K_D) against 25 cost, the sign turned by that
    of the normalisation 4 r - (r - 5).  The two sides count as equal within TIE_ULPS units in the last
    place of the larger: each is a product of doubles that stand for the decimal parameters (half a unit
    each) rounded once or twice, so a tie in real arithmetic (r = 3, cost = 0.6 at K_C - K_D = 5) is a
    tie here.  nan without a C-D bond."""
    bond_cd = split_census(row)[1].astype(np.float64)
    r, c, cost = _rcc(params)
    a, b = r * c * np.arange(-MAX_K, MAX_K + 1), 25.0 * cost
    same = np.abs(a - b) <= TIE_ULPS * 2.0 ** -53 * np.maximum(np.abs(a), abs(b))
    up = (a > b) if 4 * r - (r - 5) > 0 else (a < b)
    total = bond_cd.sum()
    if not total:
        return (float("nan"),) * 3
    return tuple(float(bond_cd[sel].sum() / total) for sel in (up & ~same, same, ~up & ~same))


def payoff_correlation_function(pairs, n, params, max_d=None):
    """Connected two-point function of the normalised payoff from one pair-sum row, d = 0 .. D: with
    Pi = (r c / 5) K - 5 cost c, (<Pi Pi'>(d) averaged over the two directions - <Pi>^2) / norm_den^2
    (the normalisation's offset drops out).  records.correlation_length applies to it as it stands."""
    pairs = np.asarray(pairs)
    D = (pairs.shape[-1] - 2) // 6 - 1 if max_d is None else int(max_d)
    sK, sc, rows, cols = split_pairs(pairs.astype(np.float64), D)
    r, c, cost = _rcc(params)
    a, b, den = r * c / 5, 5 * cost, 4 * r - (r - 5)
    t = rows + cols
    second = (a * a * t[..., 0] - a * b * t[..., 1] + b * b * t[..., 2]) / (2.0 * n)
    mean = (a * sK - b * sc) / n
    return (second - mean[..., None] ** 2) / (den * den)


@register
class Payoff(Record):
    """spgg_payoff_census of S_t: the PAYOFF_SLOTS int32 row; with D not None also spgg_payoff_pairs of
    the plane the census wrote: pairs_width(D) int64; key (every, D).

    run(payoff_every=k) records the payoff field (the census of the agents by strategy, cooperating neighbours
    and group-cooperator total K -- the payoff distribution for any parameters -- and the bonds between right /
    lower neighbours by their difference in K; with payoff_max_d also the pair sums of K and c at the distances
    0 .. payoff_max_d) on the schedule of the other records; read with payoff_histories().  Settings as for the
    other records; a function of S_t alone, so allowed on an engine that steps in persistent launches.  The
    drop-in's payoff_map_final: also the final state's per-agent map K | strategy << 5 | (m & 3) << 6 (uint8)
    as PAYOFF_MAP_DATASET."""
    name, getter, max_sides = "payoff", "payoff_histories", ("payoff_pairs",)
    options = (("payoff_history_every", "payoff_every", 0, count), ("payoff_max_distance", "payoff_max_d", None, asis),
               ("payoff_map_final", None, False, bool))
    files = specs(PAYOFF_DATASETS + (PAYOFF_PAIRS_DATASET, PAYOFF_MAP_DATASET), optional=(PAYOFF_PAIRS_DATASET, PAYOFF_MAP_DATASET),
                  payoff_values="float64", payoff_map_final="uint8")

    @staticmethod
    def validate(eng, payoff_every, payoff_max_d, what="payoff_every"):
        every, max_d = _every(what, payoff_every), payoff_max_d
        D = None if max_d is None else int(max_d)
        if D is not None and not every:
            raise ValueError("payoff_max_d needs payoff_every > 0 (nothing is recorded otherwise)")
        if D is not None:
            if eng.L > eng.payoff_pairs_max_side:
                raise ValueError(f"payoff_max_d: the device sums lattices up to side {eng.payoff_pairs_max_side}, "
                                 f"L = {eng.L} (sum snapshots on the host: payoff.host_payoff_pairs)")
            if not 0 <= D <= eng.L // 2:
                raise ValueError(f"payoff_max_d must lie in 0 .. L // 2 = {eng.L // 2}, got {D}")
        return every, D

    @classmethod
    def check_options(cls, values):
        if (values["payoff_map_final"] or values["payoff_max_distance"] is not None) and not values["payoff_history_every"]:
            raise ValueError("payoff_max_distance and payoff_map_final need payoff_history_every > 0 (nothing is "
                             "recorded otherwise)")

    @classmethod
    def finals(cls, eng, k, extras):
        return {PAYOFF_MAP_DATASET: eng.payoff_map(k)} if extras["payoff_map_final"] else {}

    def calls(self, eng):
        D, plane = self.key[1], eng._payoff_plane()
        pairs = [] if D is None else [(eng.lib.spgg_payoff_pairs, (D, plane), pairs_width(D), "int64")]
        return [(eng.lib.spgg_payoff_census, (plane,), PAYOFF_SLOTS, "int32")] + pairs   # the census first: it writes the plane

    def datasets(self, eng, k, its, r, p=None):
        d = dict(payoff_history_iters=its, payoff_census_history=r[:, :C.PAYOFF_BOND_CD].reshape((len(its),) + CENSUS_SHAPE).copy(),
                 payoff_bond_history=r[:, C.PAYOFF_BOND_CD:].copy(), payoff_values=payoff_values(eng.reps[k]))
        if p is not None:
            d[PAYOFF_PAIRS_DATASET] = p.copy()
        return d
