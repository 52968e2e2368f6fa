"""NumPy model of the strategy dwell record, written from its definitions (spgg_abi.h): flips,
since and coop are evaluated directly on the whole sequence of planes S_{t_ref} .. S_t -- not by
the per-iteration update the device (and dwell.host_dwell) apply."""
import numpy as np

AGE_BINS = 27
SLOTS = 7 + 2 * AGE_BINS
NEVER, NEVER_C, SAME, BOTH_C, NCOOP, FLIPS, COOP_TIME, AGE0 = range(8)


def fields(planes):
    """int64 (3, n) flips, age, coop of the last of the planes S_{t_ref}, .., S_t (0 = C in bit 0)."""
    P = np.stack([np.asarray(p).reshape(-1).astype(np.int64) & 1 for p in planes])   # (m, n)
    m = P.shape[0]
    flips = (P[1:] != P[:-1]).sum(axis=0)
    # since = the smallest j with S_j == .. == S_t: the run of planes equal to the last, from the end
    differs = P[::-1] != P[-1]
    run = np.where(differs.any(axis=0), differs.argmax(axis=0), m)   # its length, >= 1
    age = run - 1
    coop = (P == 0).sum(axis=0)
    return np.stack([flips, age, coop])


def bin_of(age):
    return int(age + 1).bit_length() - 1   # floor(log2(age + 1))


def row(planes):
    """The SLOTS int64 values of the last of the planes, with planes[0] the reference."""
    flips, age, coop = fields(planes)
    s = np.asarray(planes[-1]).reshape(-1).astype(np.int64) & 1
    r = np.asarray(planes[0]).reshape(-1).astype(np.int64) & 1
    out = np.zeros(SLOTS, dtype=np.int64)
    out[NEVER] = np.sum(flips == 0)
    out[NEVER_C] = np.sum((flips == 0) & (r == 0))
    out[SAME] = np.sum(s == r)
    out[BOTH_C] = np.sum((s == 0) & (r == 0))
    out[NCOOP] = np.sum(s == 0)
    out[FLIPS] = flips.sum()
    out[COOP_TIME] = coop.sum()
    ages, inverse = np.unique(age, return_inverse=True)
    np.add.at(out, AGE0 + AGE_BINS * s + np.array([bin_of(a) for a in ages])[inverse], 1)
    return out


def of_replica(planes, last, t_ref, t):
    """(row, fields) a read-out of t gives for a replica whose states S_1 .. S_last are planes[1 ..
    last] (a dict): an absorbed replica (last < t) stays at S_last."""
    seq = [planes[j] for j in range(t_ref, min(t, last) + 1)]
    return row(seq), fields(seq)


def random_planes(n, m, seed, p_flip=0.3):
    """m planes of n agents: each agent flips with probability p_flip per step (some never do)."""
    rs = np.random.RandomState(seed)
    S = rs.randint(0, 2, n)
    frozen = rs.rand(n) < 0.2
    out = [S.copy()]
    for _ in range(m - 1):
        S = S ^ ((rs.rand(n) < p_flip) & ~frozen)
        out.append(S.copy())
    return out
