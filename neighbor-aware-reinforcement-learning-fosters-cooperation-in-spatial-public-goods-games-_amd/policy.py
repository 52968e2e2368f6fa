"""The learned policy field's record: which greedy policy each agent's Q table holds, how decided
it is, and whether like-minded agents sit together (spgg_policy, spgg_abi.h).

With T the table an agent acts on at iteration t (the reference's self.q_table at the start of t;
Double-Q: the mean of its two tables), per agent

    g_s    = 0 if T[s,0] >= T[s,1] else 1     the greedy action in state s (np.argmax: ties -> 0)
    c      = g_0 + 2 g_1                      0: cooperates in both states, 1: defects in state 0 only,
                                              2: defects in state 1 only, 3: defects in both
    sigma  = the strategy S_t                 z = get_state(S_t, R_t)
    gap_s  = T[s,0] - T[s,1]

and one record row holds counts[c][sigma][z], the bonds between right / lower neighbours of one class
(bonds_same[c]) and of two (bonds_mixed), and hist[sigma][s][bins + 2] of the gaps: slot 0 the gaps
below the first edge, slots 1 .. bins np.histogram's, slot bins + 1 the gaps above the last edge.

Between two step launches the device's Q buffer is not T: it lacks the last iteration's
neighbour-influence term, which spgg_policy rebuilds on the device.  `host_policy_record` is the
NumPy model of the record given T itself; `Policy` the in-run record (the kind "policy" of records.KINDS).
"""
from __future__ import annotations

import numpy as np

from . import _lib as C
from .records import Record, _every, asis, count, register, specs

POLICY_COUNTS = C.POLICY_COUNTS     # 16 counts + 4 bonds_same + bonds_mixed
POLICY_MAX_BINS = 256

POLICY_DATASETS = ("policy_history_iters", "policy_count_history", "policy_bond_history", "policy_gap_hist_history",
                   "policy_gap_bin_edges")
POLICY_MAP_DATASET = "policy_map_final"


def policy_width(bins: int) -> int:
    """int32 slots of one record row."""
    return POLICY_COUNTS + 4 * (int(bins) + 2)


def _range(gap_range):
    """(lo, hi) of a gap range: a positive number g means (-g, g), a pair is taken as it stands."""
    try:
        lo, hi = (-float(gap_range), float(gap_range)) if np.ndim(gap_range) == 0 else map(float, gap_range)
    except (TypeError, ValueError):
        raise ValueError(f"policy gap range: a positive number or a (lo, hi) pair, got {gap_range!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"policy gap range: a positive number or a finite (lo, hi) pair with lo < hi, got {gap_range!r}")
    return lo, hi


def policy_bin_edges(gap_range=2.0, bins: int = 32) -> np.ndarray:
    """The bins + 1 edges np.histogram(x, bins=bins, range=(lo, hi)) uses; gap_range g: (-g, g)."""
    bins = int(bins)
    if not 1 <= bins <= POLICY_MAX_BINS:
        raise ValueError(f"policy bins must lie in 1 .. {POLICY_MAX_BINS}, got {bins}")
    return np.histogram_bin_edges(np.empty(0), bins, _range(gap_range))


def policy_classes(Q) -> np.ndarray:
    """The class c = g_0 + 2 g_1 of every agent of a table (.., 2, 2)."""
    Q = np.asarray(Q, dtype=np.float64)
    g = (Q[..., 0] < Q[..., 1]).astype(np.int64)      # greedy: 0 unless action 1 is strictly better
    return g[..., 0] + 2 * g[..., 1]


def policy_gap_hist(gaps, edges) -> np.ndarray:
    """bins + 2 counts of `gaps`: below edges[0], np.histogram(gaps, edges), above edges[-1]."""
    gaps, edges = np.asarray(gaps, dtype=np.float64).ravel(), np.asarray(edges, dtype=np.float64)
    return np.concatenate([[np.count_nonzero(gaps < edges[0])], np.histogram(gaps, bins=edges)[0],
                           [np.count_nonzero(gaps > edges[-1])]]).astype(np.int64)


def host_policy_record(Q, S, state, bins, edges):
    """(row, plane) of one replica on the host: the int64 row of policy_width(bins) slots and the
    uint8 plane c | sigma << 2 | z << 3, from the table Q (L, L, 2, 2) the agents act on, their
    strategies S (bit 0 counts) and their states (0 / 1), all on one (L, L) lattice.  What spgg_policy
    gives on the device."""
    Q = np.asarray(Q, dtype=np.float64)
    sigma = np.asarray(S).astype(np.int64) & 1
    z = np.asarray(state).astype(np.int64) & 1
    edges = np.asarray(edges, dtype=np.float64)
    bins = int(bins)
    if Q.shape != sigma.shape + (2, 2) or z.shape != sigma.shape or sigma.ndim != 2 or edges.shape != (bins + 1,):
        raise ValueError(f"host_policy_record: Q (L, L, 2, 2), S and state (L, L), {bins + 1} edges; got "
                         f"{Q.shape}, {sigma.shape}, {z.shape}, {edges.shape}")
    c = policy_classes(Q)
    row = np.zeros(policy_width(bins), dtype=np.int64)
    row[:16] = np.bincount((c * 4 + sigma * 2 + z).ravel(), minlength=16)
    for other in (np.roll(c, -1, axis=1), np.roll(c, -1, axis=0)):      # the right and the lower neighbour
        same = c == other
        row[16:20] += np.bincount(c[same], minlength=4)
        row[20] += np.count_nonzero(~same)
    gap = Q[..., 0] - Q[..., 1]
    hist = row[POLICY_COUNTS:].reshape(2, 2, bins + 2)
    for sg in (0, 1):
        for s in (0, 1):
            hist[sg, s] = policy_gap_hist(gap[..., s][sigma == sg], edges)
    return row, (c | sigma << 2 | z << 3).astype(np.uint8)


def split_row(row, bins):
    """(counts (.., 4, 2, 2), bonds (.., 5), hist (.., 2, 2, bins + 2)) views of record rows."""
    row = np.asarray(row)
    lead = row.shape[:-1]
    return (row[..., :16].reshape(lead + (4, 2, 2)), row[..., 16:POLICY_COUNTS],
            row[..., POLICY_COUNTS:].reshape(lead + (2, 2, int(bins) + 2)))


@register
class Policy(Record):
    """spgg_policy of iteration t: the policy_width(bins) int32 row; key (every, bins, (lo, hi)).

    run(policy_every=k) records the learned policy field (the sixteen counts class x strategy x state of the
    tables the agents act on at t -- the pending neighbour-influence term rebuilt on the device --, the bonds
    between like and unlike classes and the histograms of the two action gaps over policy_bins bins across
    policy_gap_range, a number g for (-g, g) or a (lo, hi) pair, with a slot below and one above) on the
    schedule of the other records; read with policy_histories().  Settings as for the other records; not on
    an engine that steps in persistent launches.  The drop-in's policy_map_final: also the final state's
    per-agent map class | strategy << 2 | state << 3 (uint8) as POLICY_MAP_DATASET."""
    name, getter = "policy", "policy_histories"
    options = (("policy_history_every", "policy_every", 0, count), ("policy_history_bins", "policy_bins", 32, int),
               ("policy_history_gap_range", "policy_gap_range", 2.0, asis), ("policy_map_final", None, False, bool))
    files = specs(POLICY_DATASETS + (POLICY_MAP_DATASET,), optional=(POLICY_MAP_DATASET,), policy_gap_bin_edges="float64",
                  policy_map_final="uint8")

    @staticmethod
    def validate(eng, policy_every, policy_bins, policy_gap_range, what="policy_every"):
        every, bins, gap_range = _every(what, policy_every), int(policy_bins), policy_gap_range
        if not every:
            return 0, bins, None
        if eng.persistent:
            raise ValueError(f"{what}: this engine steps in persistent launches, which have no launch boundary "
                             "between two iterations at which the table could be read")
        if not 1 <= bins <= POLICY_MAX_BINS:
            raise ValueError(f"policy_bins must lie in 1 .. {POLICY_MAX_BINS}, got {bins}")
        return every, bins, _range(gap_range)

    @classmethod
    def check_options(cls, values):
        if values["policy_map_final"] and not values["policy_history_every"]:
            raise ValueError("policy_map_final needs policy_history_every > 0 (nothing is recorded otherwise)")

    @classmethod
    def finals(cls, eng, k, extras):
        return {POLICY_MAP_DATASET: eng.policy_map(k)} if extras["policy_map_final"] else {}

    def calls(self, eng):
        _, bins, rng = self.key
        return [(eng._spgg_policy, (bins, eng._policy_edges(bins, rng), eng._policy_plane()), policy_width(bins), "int32")]

    def datasets(self, eng, k, its, r):
        _, bins, rng = self.key
        counts, bonds, hist = split_row(r, bins)
        return dict(policy_history_iters=its, policy_count_history=counts.copy(), policy_bond_history=bonds.copy(),
                    policy_gap_hist_history=hist.copy(), policy_gap_bin_edges=policy_bin_edges(rng, bins))
