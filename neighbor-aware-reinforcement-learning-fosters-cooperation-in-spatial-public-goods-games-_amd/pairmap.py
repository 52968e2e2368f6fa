"""2-D pair maps of the strategy field and of the flips of one iteration: every displacement vector
(dx, dy), not the two axes alone (spgg_pair_map, spgg_abi.h).

A field is one bit per cell of S_t: "coop" (bit 0 of the byte clear) or "flip" ((bit 0 ^ bit 3) & 1 for
t > 1, zero at t = 1: bit 3 of an S_t byte is the strategy of S_{t-1}, so the agent changed strategy in
iteration t - 1).  For two fields A, B and D <= L // 2

    map[dy][dx + D] = count_nonzero(A & np.roll(B, (-dy, -dx), axis=(0, 1)))     dy = 0 .. D, dx = -D .. D

The other half-plane is map_BA: map_AB(-dy, -dx) = map_BA(dy, dx).  From the map: the whole plane of
displacements (`full_plane`), the direction-averaged G(r) (`radial_function`) and, with D = L // 2, the
structure factor S(k) (`structure_factor`).

`host_fields` / `host_pair_map` are the NumPy models (np.roll, the definition itself; nothing of the
device's scheme); `PairMap` the in-run record (the kind "pair_map" of records.KINDS).
"""
from __future__ import annotations

import numpy as np

from . import _lib as C
from .records import Record, _every, asis, count, register, specs

FIELDS = {"coop": C.FIELD_COOP, "flip": C.FIELD_FLIP}
WORK_CAP = C.PAIR_MAP_WORK_CAP
IN_RUN_MAX_D = 32     # run()'s default distance: min(L // 2, 32)

PAIR_MAP_ITERS_DATASET = "pair_map_history_iters"
PAIR_MAP_DISTANCE_DATASET = "pair_map_max_distance"


def dataset_name(a: str, b: str) -> str:
    return f"pair_map_{a}_{b}_history"


def map_shape(D: int):
    """(D + 1, 2 D + 1): dy = 0 .. D by dx = -D .. D."""
    return (int(D) + 1, 2 * int(D) + 1)


def _distance(L, max_d, what):
    D = L // 2 if max_d is None else int(max_d)
    if not 0 <= D <= L // 2:
        raise ValueError(f"{what}: max_d must lie in 0 .. L // 2 = {L // 2}, got {max_d}")
    return D


def host_fields(S, t):
    """{"coop", "flip"}: the two bool (L, L) fields of the byte plane S of the state of iteration t
    (the bytes as the device holds them: bit 0 the strategy, bit 3 the strategy one iteration earlier;
    every other bit is masked).  The flip field of t = 1 is zero whatever bit 3 holds."""
    s = np.asarray(S).astype(np.int64)
    if s.ndim != 2 or s.shape[0] != s.shape[1]:
        raise ValueError(f"a square lattice, got {s.shape}")
    if int(t) < 1:
        raise ValueError(f"host_fields: t >= 1, got {t}")
    flip = ((s ^ (s >> 3)) & 1) == 1 if int(t) > 1 else np.zeros(s.shape, dtype=bool)
    return {"coop": (s & 1) == 0, "flip": flip}


def host_pair_map(A, B, max_d=None):
    """int64 (D + 1, 2 D + 1) pair map of two bool lattices on the host, D = max_d (None: L // 2):
    [dy, dx + D] = count_nonzero(A & np.roll(B, (-dy, -dx), axis=(0, 1))).  What spgg_pair_map counts."""
    A, B = np.asarray(A) != 0, np.asarray(B) != 0
    L = A.shape[0]
    if A.shape != (L, L) or B.shape != (L, L):
        raise ValueError(f"host_pair_map: two square lattices of one side, got {A.shape}, {B.shape}")
    D = _distance(L, max_d, "host_pair_map")
    out = np.empty(map_shape(D), dtype=np.int64)
    for dy in range(D + 1):
        By = np.roll(B, -dy, axis=0)
        for dx in range(-D, D + 1):
            out[dy, dx + D] = np.count_nonzero(A & np.roll(By, -dx, axis=1))
    return out


def host_pair_map_fft(A, B, max_d=None):
    """host_pair_map by the cross-correlation theorem (two real FFTs instead of (D + 1)(2 D + 1) rolls): the
    counts are integers below 2^31 and the rounding error of the transform far below 1/2, so the
    rounded result is the same map."""
    A, B = (np.asarray(A) != 0).astype(np.float64), (np.asarray(B) != 0).astype(np.float64)
    L = A.shape[0]
    D = _distance(L, max_d, "host_pair_map_fft")
    corr = np.fft.irfft2(np.conj(np.fft.rfft2(A)) * np.fft.rfft2(B), s=A.shape)   # [dy, dx] = sum A[y, x] B[y + dy, x + dx]
    corr = np.rint(corr).astype(np.int64)
    return corr[np.arange(D + 1)[:, None] % L, np.arange(-D, D + 1)[None, :] % L]


def work(L: int, n_rep: int, D: int) -> int:
    """The work of one spgg_pair_map call in word blocks (spgg_abi.h): every (dy, block of 32 dx) walks the
    L * ceil(L / 32) words of A once.  A call above WORK_CAP is refused."""
    L, n_rep, D = int(L), int(n_rep), int(D)
    return min(n_rep * (D + 1) * ((2 * D + 32) // 32) * L * ((L + 31) // 32), 2 ** 63 - 1)


def full_plane(m_ab, m_ba=None):
    """The (2 D + 1, 2 D + 1) map of all displacements, [dy + D, dx + D], from the stored half-plane m_ab
    and, for dy < 0, m_ba (default: m_ab, the auto-map): map_AB(-dy, -dx) = map_BA(dy, dx)."""
    m_ab = np.asarray(m_ab)
    m_ba = m_ab if m_ba is None else np.asarray(m_ba)
    D = m_ab.shape[-2] - 1
    if m_ab.shape[-2:] != map_shape(D) or m_ba.shape != m_ab.shape:
        raise ValueError(f"full_plane: maps of shape (D + 1, 2 D + 1), got {m_ab.shape}, {m_ba.shape}")
    return np.concatenate([m_ba[..., :0:-1, ::-1], m_ab], axis=-2)


def radial_function(m_ab, n, rho_a, rho_b, m_ba=None):
    """(G, count): for r = 0 .. D the mean of map / n - rho_a rho_b over the displacement vectors with
    round(hypot(dx, dy)) == r, |dx|, |dy| <= D (only the shells that lie wholly within the map are whole:
    r <= D), and the number of vectors per shell.  records.correlation_length applies to G as it stands."""
    full = full_plane(m_ab, m_ba).astype(np.float64)
    D = (full.shape[-1] - 1) // 2
    d = np.arange(-D, D + 1)
    r = np.rint(np.hypot(d[:, None], d[None, :])).astype(np.int64)
    keep = r <= D
    count = np.bincount(r[keep], minlength=D + 1)
    G = np.bincount(r[keep], weights=(full / float(n) - float(rho_a) * float(rho_b))[keep], minlength=D + 1) / count
    return G, count.astype(np.int64)


def structure_factor(m_ab, L, m_ba=None):
    """The L x L structure factor from a map with D == L // 2: the 2-D FFT of the periodic map of all L x L
    displacements over n = L * L.  For an auto-map this is |fft2(A)|^2 / n (Wiener-Khinchin), real up to
    rounding; for a cross map it is conj(fft2(A)) fft2(B) / n."""
    L = int(L)
    full = full_plane(m_ab, m_ba)
    D = (full.shape[-1] - 1) // 2
    if D != L // 2:
        raise ValueError(f"structure_factor: needs the whole plane, D == L // 2 = {L // 2}, got D = {D}")
    idx = np.arange(L)
    idx = np.where(idx <= D, idx, idx - L) + D            # displacement j -> j or j - L, as an index into full
    periodic = full[np.ix_(idx, idx)].astype(np.float64)  # [dy mod L, dx mod L]
    return np.fft.fft2(periodic) / float(L * L)


def field_pairs(fields):
    """A tuple of distinct (a, b) name pairs from run()'s pair_map_fields."""
    try:
        pairs = tuple((str(a), str(b)) for a, b in fields)
    except (TypeError, ValueError):
        raise ValueError(f"pair_map_fields: a tuple of (a, b) field name pairs, got {fields!r}") from None
    bad = [p for p in pairs if p[0] not in FIELDS or p[1] not in FIELDS]
    if bad:
        raise ValueError(f"pair_map_fields: fields are {sorted(FIELDS)}, got {bad}")
    if not pairs or len(set(pairs)) != len(pairs):
        raise ValueError(f"pair_map_fields: at least one pair and no pair twice, got {pairs}")
    return pairs


@register
class PairMap(Record):
    """spgg_pair_map of S_t, one call and one int32 tensor of (D + 1)(2 D + 1) values per field pair; key
    (every, D, fields).

    run(pair_map_every=k) records 2-D pair maps of S_t (for every displacement (dx, dy), dy = 0 .. D,
    dx = -D .. D, the cells with field a set whose partner has field b set) on the schedule of the other
    records, one map per (a, b) of pair_map_fields -- a tuple of distinct pairs of "coop" (the cooperators)
    and "flip" (the agents that changed strategy in iteration t - 1); D = pair_map_max_d, None:
    min(L // 2, 32).  A row holds (D + 1)(2 D + 1) int32 per replica and pair: 4 (D + 1)(2 D + 1) bytes, 8,580
    at D = 32 and 81,204 at D = 100.  A distance whose call would exceed the work cap (work, WORK_CAP) is
    refused; read with pair_map_histories().  Settings as for the other records; a function of S_t alone, so
    allowed on an engine that steps in persistent launches."""
    name, getter = "pair_map", "pair_map_histories"
    options = (("pair_map_history_every", "pair_map_every", 0, count), ("pair_map_max_distance", "pair_map_max_d", None, asis),
               ("pair_map_fields", "pair_map_fields", (("coop", "coop"),), lambda v: tuple(tuple(p) for p in v)))

    @staticmethod
    def validate(eng, pair_map_every, pair_map_max_d, pair_map_fields, what="pair_map_every"):
        every, max_d, fields = _every(what, pair_map_every), pair_map_max_d, pair_map_fields
        if not every:
            return 0, None, ()
        D = min(eng.L // 2, IN_RUN_MAX_D) if max_d is None else int(max_d)
        if not 0 <= D <= eng.L // 2:
            raise ValueError(f"pair_map_max_d must lie in 0 .. L // 2 = {eng.L // 2}, got {D}")
        pairs = field_pairs(fields)
        w = max(work(eng.L, g["r1"] - g["r0"], D) for g in eng.groups)
        if w > WORK_CAP:
            raise ValueError(f"pair_map_max_d = {D}: one call would be {w} word blocks, above the cap {WORK_CAP} "
                             "(pairmap.work; a smaller distance, or map snapshots on the host: pairmap.host_pair_map)")
        return every, D, pairs

    @classmethod
    def check_options(cls, values):
        if values["pair_map_max_distance"] is not None and not values["pair_map_history_every"]:
            raise ValueError("pair_map_max_distance needs pair_map_history_every > 0 (nothing is recorded otherwise)")
        values["pair_map_fields"] = field_pairs(values["pair_map_fields"])

    @classmethod
    def file_datasets(cls, hist):
        """The iterations, one map per field pair (the key's pairs: the names datasets gave them), the distance."""
        maps = [name for name in hist if name not in (PAIR_MAP_ITERS_DATASET, PAIR_MAP_DISTANCE_DATASET)]
        return specs([PAIR_MAP_ITERS_DATASET, *maps, PAIR_MAP_DISTANCE_DATASET])

    def calls(self, eng):
        _, D, pairs = self.key
        ws = eng._pair_map_work(D)
        width = map_shape(D)[0] * map_shape(D)[1]
        return [(eng.lib.spgg_pair_map, (FIELDS[a], FIELDS[b], D, ws), width, "int32") for a, b in pairs]

    def datasets(self, eng, k, its, *rows):
        _, D, pairs = self.key
        d = {PAIR_MAP_ITERS_DATASET: its, PAIR_MAP_DISTANCE_DATASET: np.int64(D)}
        for (a, b), r in zip(pairs, rows):
            d[dataset_name(a, b)] = r.reshape((len(its),) + map_shape(D)).copy()
        return d
