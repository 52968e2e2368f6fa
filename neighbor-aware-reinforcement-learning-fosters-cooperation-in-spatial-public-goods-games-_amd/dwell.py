"""The per-agent strategy dwell record: persistence, two-time autocorrelation, strategy ages and
cooperation frequency (spgg_dwell_*, spgg_abi.h).

Unlike the other kinds of records.KINDS this one is not a function of one instant: the device carries
three words per agent from one iteration to the next (BatchEngine.dwell_start), and `Dwell` is the
in-run read-out of them on the schedule of every other record; its two hooks start and stop the
tracking.  With tracking started at t_ref (strategy = bit 0 of S, 0 = C):

    flips_i(t)  the number of j in t_ref .. t-1 with S_{j+1}[i] != S_j[i]
    since_i(t)  the smallest j >= t_ref with S_j[i] == .. == S_t[i];  age_i(t) = t - since_i(t)
    coop_i(t)   the number of j in t_ref .. t with S_j[i] == C
"""
from __future__ import annotations

import numpy as np

from . import _lib as C
from .records import Record, _every, count, register, specs

DWELL_AGE_BINS = C.DWELL_AGE_BINS   # age bin b = floor(log2(age + 1)), 0 .. 26 (age + 1 <= 2^26)
DWELL_SLOTS = C.DWELL_SLOTS         # 7 counts and sums, then the 2 x DWELL_AGE_BINS age histogram

DWELL_DATASETS = ("dwell_history_iters", "dwell_ref_iteration", "persistence_history", "autocorrelation_history",
                  "flip_total_history", "cooperator_time_history", "strategy_age_hist_history")
DWELL_FIELD_DATASETS = ("flip_count_final", "strategy_age_final", "cooperation_frequency_final")


def age_bin_edges() -> np.ndarray:
    """The DWELL_AGE_BINS + 1 integer edges of the age histogram: bin b holds the ages
    2^b - 1 <= age < 2^(b+1) - 1."""
    return (1 << np.arange(DWELL_AGE_BINS + 1, dtype=np.int64)) - 1


def age_bin(age) -> np.ndarray:
    """floor(log2(age + 1)) of non-negative integer ages, exactly."""
    return np.searchsorted(age_bin_edges(), np.asarray(age, dtype=np.int64), side="right") - 1


def persistence(never, n):
    """The share of agents that have not changed strategy since the reference iteration."""
    return np.asarray(never, dtype=np.float64) / n


def autocorrelation(same, n):
    """<s_i(t_ref) s_i(t)> with s = +-1, from the number of agents whose strategy is the
    reference's: 2 same / n - 1."""
    return 2.0 * np.asarray(same, dtype=np.float64) / n - 1.0


def dwell_row(S, ref, flips, age, coop) -> np.ndarray:
    """The DWELL_SLOTS int64 row (spgg_abi.h) of one replica from its current and reference
    strategies (0/1) and its per-agent fields, all of one shape."""
    s, r = np.asarray(S).ravel() & 1, np.asarray(ref).ravel() & 1
    flips, age, coop = (np.asarray(x, dtype=np.int64).ravel() for x in (flips, age, coop))
    row = np.zeros(DWELL_SLOTS, dtype=np.int64)
    row[C.DW_NEVER] = np.count_nonzero(flips == 0)
    row[C.DW_NEVER_C] = np.count_nonzero((flips == 0) & (r == 0))
    row[C.DW_SAME] = np.count_nonzero(s == r)
    row[C.DW_BOTH_C] = np.count_nonzero((s == 0) & (r == 0))
    row[C.DW_NCOOP] = np.count_nonzero(s == 0)
    row[C.DW_FLIPS] = flips.sum()
    row[C.DW_COOP_TIME] = coop.sum()
    row[C.DW_AGE0:] = np.bincount(s * DWELL_AGE_BINS + age_bin(age), minlength=2 * DWELL_AGE_BINS)
    return row


def host_dwell(planes, t_ref: int = 1):
    """(row, fields) of the last of the S planes S_{t_ref}, S_{t_ref + 1}, .., S_t (a list of equally
    shaped integer arrays; only bit 0 counts): the DWELL_SLOTS int64 row and the int64 fields
    (3, *shape) flips, age, coop -- by the update the device applies after every step launch, on
    the host: an agent's words change only when it flips.  What spgg_dwell_record and
    spgg_dwell_fields give for a replica that has not been absorbed before t."""
    planes = [np.asarray(p).astype(np.int64) & 1 for p in planes]
    if not planes:
        raise ValueError("host_dwell: at least the reference plane S_{t_ref}")
    prev = planes[0]
    flips, closed = np.zeros_like(prev), np.zeros_like(prev)
    since = np.full_like(prev, t_ref)
    for j, cur in enumerate(planes[1:], start=int(t_ref)):   # the launch of iteration j made cur = S_{j+1}
        flipped = cur != prev
        flips[flipped] += 1
        ended = flipped & (prev == 0)
        closed[ended] += (j + 1) - since[ended]
        since[flipped] = j + 1
        prev = cur
    t = int(t_ref) + len(planes) - 1
    age = t - since
    coop = closed + np.where(prev == 0, age + 1, 0)
    return dwell_row(prev, planes[0], flips, age, coop), np.stack([flips, age, coop])


_FIELDS = ("flip_count", "strategy_age", "cooperation_frequency")      # BatchEngine.dwell_fields' keys, as DWELL_FIELD_DATASETS


@register
class Dwell(Record):
    """spgg_dwell_record of S_t: the DWELL_SLOTS int64 row; t0 is the reference iteration, at which
    BatchEngine.run starts the tracking; key (every,).

    run(dwell_every=k) also tracks the per-agent strategy dwell record (dwell_start at the run's first
    iteration, the reference: one more launch after every step launch) and records its row (persistence,
    autocorrelation, flips, cooperator time, strategy ages) on the schedule of the other records; read with
    dwell_histories().  A run continued with the same k keeps its record and its reference, another k starts
    afresh at the current t, 0 stops the tracking of an earlier run and drops its record; not on an engine that
    steps in persistent launches.  The drop-in's dwell_fields: also the per-agent DWELL_FIELD_DATASETS of the
    final state."""
    name, getter = "dwell", "dwell_histories"
    options = (("dwell_history_every", "dwell_every", 0, count), ("dwell_fields", None, False, bool))
    files = specs(DWELL_DATASETS + DWELL_FIELD_DATASETS, optional=DWELL_FIELD_DATASETS, cooperation_frequency_final="float64")

    def __init__(self, every, t0, T, key=None):
        super().__init__(every, t0, T, (int(every),))

    @staticmethod
    def validate(eng, dwell_every):
        every = _every("dwell_every", dwell_every)
        if every and eng.persistent:
            raise ValueError("dwell_every: this engine steps in persistent launches, which have no launch "
                             "boundary between two iterations for the dwell launch")
        return (every,)

    @classmethod
    def starting(cls, eng):
        """The tracking (re)starts with the new record.  dwell_start and dwell_stop drop the record, so one that
        is still there has t0 == eng.dwell_t_ref: it is kept exactly if `every` matches."""
        eng.dwell_start()

    @classmethod
    def unasked(cls, eng):
        eng.dwell_stop()

    @classmethod
    def check_options(cls, values):
        if values["dwell_fields"] and not values["dwell_history_every"]:
            raise ValueError("dwell_fields needs dwell_history_every > 0 (nothing is tracked otherwise)")

    @classmethod
    def finals(cls, eng, k, extras):
        if not extras["dwell_fields"]:
            return {}
        f = eng.dwell_fields(k)
        return {name: f[key] for name, key in zip(DWELL_FIELD_DATASETS, _FIELDS)}

    def calls(self, eng):
        return [(eng.lib.spgg_dwell_record, (), DWELL_SLOTS, "int64")]

    def datasets(self, eng, k, its, r):
        return dict(dwell_history_iters=its, dwell_ref_iteration=np.int64(self.t0),
                    persistence_history=r[:, [C.DW_NEVER, C.DW_NEVER_C]].copy(),
                    autocorrelation_history=r[:, [C.DW_SAME, C.DW_BOTH_C, C.DW_NCOOP]].copy(),
                    flip_total_history=r[:, C.DW_FLIPS].copy(), cooperator_time_history=r[:, C.DW_COOP_TIME].copy(),
                    strategy_age_hist_history=r[:, C.DW_AGE0:].reshape(len(its), 2, DWELL_AGE_BINS).copy())
