"""The in-run device records of BatchEngine.run and the host-side models of what they hold.

A `Record` is one stream of observations of the running lattice: every `every` iterations from `t0`
on, one ABI call per device tensor writes one row.  The kinds (KINDS, the registry of all of them) differ
only in their class data -- options and datasets -- and in their settings, calls and rows.  The schedule
is plain Python; the engine allocates and enqueues (_observe).
"""
from __future__ import annotations

import numpy as np

from . import _lib as C

KINDS = {}      # name -> kind, in the order the kinds' datasets have in the file (register)


def register(kind):
    """Class decorator: enter a kind into KINDS.  clusters, correlations and reputation register here, dwell,
    policy, payoff and pair_map in their own modules, which engine.py imports in that order."""
    KINDS[kind.name] = kind
    return kind


def next_boundary(t, stops, check_at, end, records=()):
    """The iteration at which the turn of BatchEngine.run that starts at t ends: the next snapshot /
    PNG stop, the next stop-flag copy (check_at), the run's end (T + 1) or the next row of an active
    record, whichever comes first."""
    return min([s for s in stops if s > t] + [check_at, end] + [r.next_due(t) for r in records])


def _every(name, value) -> int:
    value = int(value)
    if value < 0:
        raise ValueError(f"{name} must be >= 0")
    return value


def count(v) -> int:
    """An *_every option of the drop-in: None and 0 switch the record off."""
    return int(v or 0)


def asis(v):
    return v


def specs(names, optional=(), **dtypes):
    """A kind's `files` from dataset names in file order: int64 unless `dtypes` says float64 or uint8."""
    return tuple((name, dtypes.get(name, "int64"), name in optional) for name in names)


class Record:
    """A record of the iterations t0, t0 + every, ... <= T: `key` its settings (every first), `out`
    its device tensors, each (R, rows, width) with one row per recorded iteration, `plan` the (ABI
    function, its scalar arguments, width, dtype) of the call that fills each (a kind's calls).

    A kind states as class data what its callers need: `name` (its key in KINDS and BatchEngine.records),
    `getter` (BatchEngine's *_histories method), `options` -- one (drop-in attribute, BatchEngine.run keyword
    or None for an option of the drop-in alone, default, conversion) each, the *_every option first --, `files`
    -- one (dataset, dtype, optional) each, in file order -- and `max_sides`, the x of the spgg_<x>_max_side
    entry points its validate reads as eng.<x>_max_side.  validate(eng, **its run keywords) -> key raises the
    ValueErrors of run(); calls(eng) is the plan; datasets(eng, k, its, *rows) one replica's history."""
    name = getter = None
    options = files = max_sides = ()

    def __init__(self, every, t0, T, key=()):
        self.every, self.t0, self.key = int(every), int(t0), key
        self.rows = max(1, (T - self.t0) // self.every + 1)
        self.plan, self.out = [], []

    def due(self, t) -> bool:
        return (t - self.t0) % self.every == 0

    def next_due(self, t) -> int:
        """The first recorded iteration after t."""
        return t + self.every - (t - self.t0) % self.every

    def row(self, t) -> int:
        return (t - self.t0) // self.every

    def iters(self, last) -> np.ndarray:
        return np.arange(self.t0, last + 1, self.every, dtype=np.int64)

    def write(self, eng, t):
        """Enqueue the record of iteration t into its row of every tensor."""
        row = self.row(t)
        for (fn, args, width, _), out in zip(self.plan, self.out):
            eng._observe(fn, t, args, out, row * width)

    def histories(self, eng):
        """Per replica, the datasets of the recorded iterations t <= last_iteration (so a replica
        absorbed at s keeps the record of S_s if s was recorded)."""
        host = [o.cpu().numpy().astype(np.int64, copy=False) for o in self.out]
        its = [self.iters(eng.last_iteration(k)) for k in range(eng.R)]
        return [self.datasets(eng, k, its[k], *[h[k, :len(its[k])] for h in host]) for k in range(eng.R)]

    # -- what a kind may add (dwell.Dwell has the first two; no kind needs all) --
    @classmethod
    def starting(cls, eng):
        """BatchEngine.run is about to create a new record of the kind."""

    @classmethod
    def unasked(cls, eng):
        """BatchEngine.run was asked for the kind with every == 0 while an earlier run's record exists (which
        stays readable unless the kind drops it here)."""

    @classmethod
    def check_options(cls, values):
        """The drop-in's cross-checks (ValueError) of the kind's converted option values, attribute -> value;
        may normalise them in place."""

    @classmethod
    def finals(cls, eng, k, extras) -> dict:
        """The final-state datasets of replica k that the drop-in-only options `extras` ask for."""
        return {}

    @classmethod
    def file_datasets(cls, hist):
        """`files` of one replica's history."""
        return cls.files


def clusters_tile(tiled):
    """The tile side a clusters_tiled value asks for: False -> None (the one-workgroup LDS kernel),
    True -> 0 (the library's tile), an int -> that side, 8 .. 200."""
    if tiled is False or tiled is None:
        return None
    if tiled is True:
        return 0
    tile = int(tiled)
    if not C.CLUSTERS_TILE_MIN <= tile <= C.CLUSTERS_TILE_MAX:
        raise ValueError(f"clusters_tiled: a tile side in {C.CLUSTERS_TILE_MIN} .. {C.CLUSTERS_TILE_MAX} "
                         f"(or True for the library's, {C.CLUSTERS_TILE_DEFAULT}), got {tiled!r}")
    return tile


def clusters_cap_text(tiled) -> str:
    """What a cluster count of -1 means, by the path that wrote it."""
    if not tiled:
        return f"the labelling's pass cap ({C.CLUSTERS_MAX_PASSES})"
    return (f"a cap of the tiled labelling (a tile's pass cap {C.CLUSTERS_MAX_PASSES}, a root walk of n steps or "
            f"a seam union's retry cap {C.CLUSTERS_TILED_MAX_RETRIES})")


def _tiled(v):
    return v if isinstance(v, bool) else (int(v) if v else False)


CLUSTER_DATASETS = ("cluster_history_iters", "cluster_count_history", "largest_cluster_history", "cd_bond_history")
CORRELATION_DATASETS = ("correlation_history_iters", "pair_count_rows_history", "pair_count_cols_history")
# the last four only with reputation_max_distance set (BatchEngine.reputation_histories)
REPUTATION_DATASETS = ("reputation_history_iters", "reputation_hist_history", "reputation_bin_edges",
                       "reputation_sum_history", "reputation_pair_rows_history", "reputation_pair_cols_history",
                       "reputation_unit")


@register
class Clusters(Record):
    """spgg_clusters of S_t: (clusters, largest cluster, C-D bonds) int32; key (every, periodic, tile): tile
    None for the one-workgroup LDS kernel, else the tile side of spgg_clusters_tiled (0: the library's).

    run(clusters_every=k): the number of cooperator clusters, the largest cluster and the C-D bonds;
    clusters_periodic: of the wrapped lattice (the drop-in's final cluster_sizes dataset never wraps:
    spgg.py:631); read with cluster_histories().  clusters_tiled: False: the one-workgroup LDS kernel, lattices
    up to clusters_max_side; True: spgg_clusters_tiled (one replica over many workgroups, any side) with the
    library's tile; an int: with that tile side (8 .. 200).  Same record either way; part of the record's
    settings; needs clusters_every > 0."""
    name, getter, max_sides = "clusters", "cluster_histories", ("clusters",)
    options = (("cluster_history_every", "clusters_every", 0, count),
               ("cluster_history_periodic", "clusters_periodic", False, bool),
               ("cluster_history_tiled", "clusters_tiled", False, _tiled))
    files = specs(CLUSTER_DATASETS)

    @staticmethod
    def validate(eng, clusters_every, clusters_periodic, clusters_tiled=False):
        every, periodic = _every("clusters_every", clusters_every), clusters_periodic
        tile = clusters_tile(clusters_tiled)
        if tile is not None and not every:
            raise ValueError("clusters_tiled needs clusters_every > 0 (nothing is recorded otherwise)")
        if every and tile is None and eng.L > eng.clusters_max_side:
            raise ValueError(f"clusters_every: the one-workgroup kernel labels lattices up to side {eng.clusters_max_side}, "
                             f"L = {eng.L} (clusters_tiled=True records any side; or label snapshots on the host: "
                             "engine.host_cluster_sizes)")
        return every, bool(periodic), tile

    def calls(self, eng):
        _, periodic, tile = self.key
        if tile is None:
            return [(eng.lib.spgg_clusters, (int(periodic), None), 3, "int32")]
        return [(eng.lib.spgg_clusters_tiled, (int(periodic), tile, eng._clusters_workspace(), None), 3, "int32")]

    def datasets(self, eng, k, its, r):
        if np.any(r[:, 0] < 0):
            tiled = self.key[2] is not None
            raise C.SpggError(f"{'spgg_clusters_tiled' if tiled else 'spgg_clusters'}: replica {k} ran into "
                              f"{clusters_cap_text(tiled)} at iterations {its[r[:, 0] < 0].tolist()}")
        return dict(cluster_history_iters=its, cluster_count_history=r[:, 0].copy(),
                    largest_cluster_history=r[:, 1].copy(), cd_bond_history=r[:, 2].copy())


@register
class Correlations(Record):
    """spgg_correlations of S_t: D + 1 row then D + 1 column pair counts, int32; key (every, D).

    run(correlations_every=k): the cooperator pair counts along rows and columns at the distances
    0 .. correlations_max_d (None: L // 2); read with correlation_histories()."""
    name, getter, max_sides = "correlations", "correlation_histories", ("correlations",)
    options = (("correlation_history_every", "correlations_every", 0, count),
               ("correlation_max_distance", "correlations_max_d", None, asis))
    files = specs(CORRELATION_DATASETS)

    @staticmethod
    def validate(eng, correlations_every, correlations_max_d):
        every, max_d = _every("correlations_every", correlations_every), correlations_max_d
        D = eng.L // 2 if max_d is None else int(max_d)
        if every and not 0 <= D <= eng.L // 2:
            raise ValueError(f"correlations_max_d must lie in 0 .. L // 2 = {eng.L // 2}, got {D}")
        if every and eng.L > eng.correlations_max_side:
            raise ValueError(f"correlations_every: the device counts lattices up to side {eng.correlations_max_side}, "
                             f"L = {eng.L} (count snapshots on the host: engine.host_pair_counts)")
        return every, D

    def calls(self, eng):
        return [(eng.lib.spgg_correlations, (self.key[1],), 2 * (self.key[1] + 1), "int32")]

    def datasets(self, eng, k, its, r):
        D = self.key[1]
        return dict(correlation_history_iters=its, pair_count_rows_history=r[:, :D + 1].copy(),
                    pair_count_cols_history=r[:, D + 1:].copy())


@register
class Reputation(Record):
    """spgg_reputation_hist of (S_t, R_t): 2 x bins counts, int32, over each replica's reference edges; with
    D not None also spgg_reputation_pairs of the int8 plane: sum, D + 1 row and D + 1 column sums,
    int64; key (every, bins, D).

    run(reputation_every=k): the joint histogram strategy x bin (reputation_bins bins over each replica's
    R_min .. R_max, the reference's edges); with reputation_max_d also the pair sums of the int8 reputation
    plane at the distances 0 .. reputation_max_d (not on an f64-reputation engine or above
    reputation_max_side); read with reputation_histories()."""
    name, getter, max_sides = "reputation", "reputation_histories", ("reputation",)
    options = (("reputation_history_every", "reputation_every", 0, count),
               ("reputation_history_bins", "reputation_bins", 20, int),
               ("reputation_max_distance", "reputation_max_d", None, asis))
    files = specs(REPUTATION_DATASETS, optional=REPUTATION_DATASETS[3:], reputation_bin_edges="float64",
                  reputation_unit="float64")

    @staticmethod
    def validate(eng, reputation_every, reputation_bins, reputation_max_d):
        every, bins, max_d = _every("reputation_every", reputation_every), int(reputation_bins), reputation_max_d
        D = None if max_d is None else int(max_d)
        if every and not 1 <= bins <= 256:
            raise ValueError(f"reputation_bins must lie in 1 .. 256, got {bins}")
        if every and D is not None:
            if not eng.rep_int8:
                raise ValueError("reputation_max_d: the pair sums are exact integers of the int8 reputation path; "
                                 "this engine holds f64 reputation (non-dyadic gains or bounds) -- sum snapshots "
                                 "on the host: engine.host_reputation_pair_sums")
            if eng.L > eng.reputation_max_side:
                raise ValueError(f"reputation_max_d: the device sums lattices up to side {eng.reputation_max_side}, "
                                 f"L = {eng.L} (sum snapshots on the host: engine.host_reputation_pair_sums)")
            if not 0 <= D <= eng.L // 2:
                raise ValueError(f"reputation_max_d must lie in 0 .. L // 2 = {eng.L // 2}, got {D}")
        return every, bins, D

    def calls(self, eng):
        _, bins, D = self.key
        pairs = [] if D is None else [(eng.lib.spgg_reputation_pairs, (D,), 2 * (D + 1) + 1, "int64")]
        return [(eng.lib.spgg_reputation_hist, (bins, eng._reputation_edges(bins)), 2 * bins, "int32")] + pairs

    def datasets(self, eng, k, its, h, r=None):
        _, bins, D = self.key
        d = dict(reputation_history_iters=its, reputation_hist_history=h.reshape(len(its), 2, bins).copy(),
                 reputation_bin_edges=reputation_bin_edges(eng.reps[k].R_min, eng.reps[k].R_max, bins))
        if r is not None:
            d.update(reputation_sum_history=r[:, 0].copy(), reputation_pair_rows_history=r[:, 1:D + 2].copy(),
                     reputation_pair_cols_history=r[:, D + 2:].copy(), reputation_unit=np.float64(eng.rep_units[k]))
        return d


def host_cluster_sizes(S, periodic: bool = False) -> np.ndarray:
    """int64 sizes of the 4-connected cooperator (S == 0) clusters of one lattice in label order
    (ascending smallest raster index), on the host: scipy.ndimage.label (spgg.py:631-633);
    periodic merges its labels across the two seams.  The path of lattices above the device
    labelling's supported side (spgg_clusters_max_side)."""
    from scipy.ndimage import label
    lab, k = label(np.asarray(S) == 0)
    counts = np.bincount(lab.ravel(), minlength=k + 1).astype(np.int64)
    if not periodic or k == 0:
        return counts[1:]
    root = np.arange(k + 1)

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for a, b in list(zip(lab[0], lab[-1])) + list(zip(lab[:, 0], lab[:, -1])):
        if a and b:
            ra, rb = find(a), find(b)
            if ra != rb:
                root[max(ra, rb)] = min(ra, rb)   # the label met first in raster order stays
    owner = np.array([find(a) for a in range(k + 1)])
    merged = np.bincount(owner, weights=counts, minlength=k + 1).astype(np.int64)
    return merged[(owner == np.arange(k + 1)) & (np.arange(k + 1) > 0)]


def host_pair_counts(S, max_d=None) -> np.ndarray:
    """int64 (2, D+1) cooperator pair counts of one lattice on the host, D = max_d (None: L // 2):
    with c = 1 where bit 0 of S is 0, [0, d] = sum(c & roll(c, -d, axis=1)) (pairs d apart along
    a row) and [1, d] = sum(c & roll(c, -d, axis=0)) (along a column), periodic.  What
    spgg_correlations counts on the device, and the path of lattices above its supported side
    (spgg_correlations_max_side)."""
    c = (np.asarray(S).astype(np.int64) & 1) == 0
    L = c.shape[0]
    D = L // 2 if max_d is None else int(max_d)
    if c.shape != (L, L) or D < 0 or D > L // 2:
        raise ValueError(f"host_pair_counts: a square lattice and 0 <= max_d <= L // 2, got {c.shape}, {max_d}")
    out = np.empty((2, D + 1), dtype=np.int64)
    for d in range(D + 1):
        out[0, d] = np.count_nonzero(c & np.roll(c, -d, axis=1))
        out[1, d] = np.count_nonzero(c & np.roll(c, -d, axis=0))
    return out


def correlation_function(rows, cols, n):
    """Connected two-point function of the cooperator field from pair counts (any leading axes,
    the distance last): G(d) = (rows + cols) / (2 n) - (rows[..., 0] / n)^2, n = L * L cells --
    the direction-averaged <c(x) c(x + d)> minus the squared cooperation rate."""
    rows, cols = np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.float64)
    rho = rows[..., :1] / n
    return (rows + cols) / (2.0 * n) - rho * rho


def correlation_length(G) -> float:
    """Distance at which g = G / G[0] first falls to 1/e: the first d >= 1 with g(d) <= 1/e,
    linearly interpolated between d - 1 and d.  nan if G[0] == 0 (an absorbed lattice), inf if g
    never falls that far within the given distances."""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 1 or G.size == 0:
        raise ValueError("correlation_length: a one-dimensional G(d), d = 0 ..")
    if G[0] == 0:
        return float("nan")
    g = G / G[0]
    below = np.nonzero(g[1:] <= 1.0 / np.e)[0]
    if below.size == 0:
        return float("inf")
    d = int(below[0]) + 1
    return float(d - 1 + (g[d - 1] - 1.0 / np.e) / (g[d - 1] - g[d]))


def reputation_bin_edges(R_min, R_max, bins: int = 20) -> np.ndarray:
    """The bins + 1 edges np.histogram(x, bins=bins, range=(R_min, R_max)) uses -- with bins = 20
    the reference's rep_bins_* datasets (spgg.py:399)."""
    return np.histogram_bin_edges(np.empty(0), int(bins), (float(R_min), float(R_max)))


def host_reputation_pair_sums(K, max_d=None):
    """(sum, rows, cols) of one reputation lattice on the host, D = max_d (None: L // 2): sum =
    K.sum(), rows[d] = sum(K * roll(K, -d, axis=1)), cols[d] = sum(K * roll(K, -d, axis=0)) for
    d = 0 .. D, periodic.  Integer input (the int8 plane, in units of rep_unit) is summed in int64
    and is what spgg_reputation_pairs gives on the device, exactly; float input (R itself, the f64
    reputation path) gives the same sums in float64, rounded and so not exact.  The path of
    f64-reputation engines and of lattices above spgg_reputation_max_side."""
    K = np.asarray(K)
    L = K.shape[0]
    D = L // 2 if max_d is None else int(max_d)
    if K.shape != (L, L) or D < 0 or D > L // 2:
        raise ValueError(f"host_reputation_pair_sums: a square lattice and 0 <= max_d <= L // 2, got {K.shape}, {max_d}")
    K = K.astype(np.int64 if np.issubdtype(K.dtype, np.integer) else np.float64)
    rows, cols = np.empty(D + 1, dtype=K.dtype), np.empty(D + 1, dtype=K.dtype)
    for d in range(D + 1):
        rows[d] = np.sum(K * np.roll(K, -d, axis=1))
        cols[d] = np.sum(K * np.roll(K, -d, axis=0))
    return K.sum(), rows, cols


def reputation_correlation_function(sum, rows, cols, n, unit):
    """Connected two-point function of the reputation field from pair sums (any leading axes, the
    distance last; sum without the distance axis): unit^2 * ((rows + cols) / (2 n) - (sum / n)^2),
    n = L * L cells, unit the replica's rep_unit (1 for sums of R itself) -- the direction-averaged
    <R(x) R(x + d)> minus the squared mean.  correlation_length applies to it as it stands."""
    rows, cols = np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.float64)
    mean = np.asarray(sum, dtype=np.float64)[..., None] / n
    return float(unit) ** 2 * ((rows + cols) / (2.0 * n) - mean * mean)

