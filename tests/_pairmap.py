"""Shared by the pair-map tests: the synthetic byte planes (strategy in bit 0, a chosen previous strategy
in bit 3, every other bit random), the oracle's side of the in-run record, and a NumPy model of the
device's own scheme (csrc/spgg_pair_map.hip: field A as plain bit rows, field B as extended rows whose
bit j is B[(j - D) mod L], the two-word funnel, 32-wide dx blocks of which the last is cut at 2 D).
NumPy only."""
import numpy as np

from spgg_amd import pairmap as PM

WORD = 32
BLOCK = 32                                    # spgg_pm::kBlock
SMALL_WORDS, FULL_WORDS = 16384 // 4, 163840 // 4      # spgg_pm::kSmallWords, kFullWords
PAIRS = (("coop", "coop"), ("flip", "flip"), ("coop", "flip"))
ALL_PAIRS = PAIRS + (("flip", "coop"),)
KEEP = 0x09                                   # the bits the fields read


# ---- the device's layout ---------------------------------------------------------------------------------------------
def row_words(L):
    return (L + WORD - 1) // WORD


def ext_words(L, D):
    return (L + 2 * D + WORD - 1) // WORD + 1


def plane_words(L, D):
    """spgg_pm::plane_words: what spgg_pair_map_workspace returns per replica."""
    return L * (row_words(L) + ext_words(L, D))


def dx_blocks(D):
    return (2 * D + BLOCK) // BLOCK


def instance(L, D):
    """Which count instance the host picks: "small" (16 KiB of LDS), "full" (160 KiB) or "global"."""
    w = plane_words(L, D)
    return "small" if w <= SMALL_WORDS else "full" if w <= FULL_WORDS else "global"


def instance_edges(D):
    """[(last side of an instance, first side of the next)] at distance D."""
    out, L = [], max(2 * D, 1)
    while len(out) < 2:
        if instance(L, D) != instance(L + 1, D):
            out.append((L, L + 1))
        L += 1
    return out


def _pack(bits):
    """(rows, nbits) bool -> (rows, words) uint64 holding 32-bit words, bit x & 31 of word x >> 5."""
    rows, nbits = bits.shape
    words = (nbits + WORD - 1) // WORD
    padded = np.zeros((rows, words * WORD), dtype=np.uint64)
    padded[:, :nbits] = bits
    weights = np.uint64(1) << np.arange(WORD, dtype=np.uint64)
    return (padded.reshape(rows, words, WORD) * weights).sum(axis=2, dtype=np.uint64)


def pack_plain(A):
    return _pack(np.asarray(A) != 0)


def pack_extended(B, D):
    """Extended rows: bit j = B[y][(j - D) mod L] for j < L + 2 D, zero up to whole words, one more zero word."""
    B = np.asarray(B) != 0
    L = B.shape[0]
    ext = B[:, (np.arange(L + 2 * D) - D) % L]
    packed = _pack(ext)
    out = np.zeros((L, ext_words(L, D)), dtype=np.uint64)
    out[:, :packed.shape[1]] = packed
    assert packed.shape[1] == ext_words(L, D) - 1
    return out


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _popcount32(v):
    v = v.astype(np.uint64)
    return sum(_POP8[((v >> np.uint64(s)) & np.uint64(0xff)).astype(np.int64)] for s in (0, 8, 16, 24))


def model_pair_map(A, B, D):
    """The map as the count launch forms it."""
    L = np.asarray(A).shape[0]
    W = row_words(L)
    pa, pe = pack_plain(A), pack_extended(B, D)
    out = np.full(PM.map_shape(D), -1, dtype=np.int64)
    w = np.arange(W)
    for dy in range(D + 1):
        rolled = pe[(np.arange(L) + dy) % L]
        for b in range(dx_blocks(D)):
            assert w[-1] + b + 1 <= pe.shape[1] - 1          # the second word of the last window exists
            lo, hi = rolled[:, w + b], rolled[:, w + b + 1]
            both = (hi << np.uint64(32)) | lo
            for j in range(BLOCK):
                col = BLOCK * b + j
                if col > 2 * D:
                    break
                window = (both >> np.uint64(j)) & np.uint64(0xffffffff)
                out[dy, col] = _popcount32(pa & window).sum()
    assert out.min() >= 0
    return out


# ---- synthetic planes ------------------------------------------------------------------------------------------------
def byte_plane(S, prev, seed):
    """uint8 plane: strategy S in bit 0, prev in bit 3, bits 1, 2 and 4-7 random."""
    rs = np.random.RandomState(seed)
    noise = rs.randint(0, 256, np.shape(S)).astype(np.uint8) & np.uint8(0xff ^ KEEP)
    return ((np.asarray(S).astype(np.uint8) & 1) | ((np.asarray(prev).astype(np.uint8) & 1) << 3) | noise).astype(np.uint8)


def l_figure(L):
    """An asymmetric figure (an L: a bar down and a foot to the right) on an empty lattice, bool."""
    F = np.zeros((L, L), dtype=bool)
    y0, x0 = L // 4, L // 3
    for k in range(min(3, L)):
        F[(y0 + k) % L, x0 % L] = True
    F[(y0 + min(2, L - 1)) % L, (x0 + 1) % L] = True
    return F


def patterns(L, seed=0):
    """{name: (S, prev)} int64 (L, L), 0 = C: a random plane at cooperator density 0.4 with the last three
    columns empty and the last two rows full (flips at random), a checkerboard (flips in stripes), all-C
    (one flip), all-D (no flip), one cooperator (flips: the L figure)."""
    rs = np.random.RandomState(5000 + 13 * L + seed)
    y, x = np.mgrid[0:L, 0:L]
    coop = rs.rand(L, L) < 0.4
    coop[:, -3:] = False
    coop[-2:, :] = True
    rnd = 1 - coop.astype(np.int64)
    one_flip = np.zeros((L, L), dtype=np.int64)
    one_flip[(2 * L) // 3, L // 5] = 1
    one_c = np.ones((L, L), dtype=np.int64)
    one_c[L // 3, (2 * L) // 3] = 0
    return {
        "random": (rnd, rnd ^ (rs.rand(L, L) < 0.3)),
        "checkerboard": ((x + y) & 1, x & 1),
        "all_c": (np.zeros((L, L), dtype=np.int64), one_flip),
        "all_d": (np.ones((L, L), dtype=np.int64), np.ones((L, L), dtype=np.int64)),
        "one_cell": (one_c, one_c ^ l_figure(L)),
    }


def smaller(L):
    """One distance below L // 2 (0 where there is none)."""
    D = L // 2
    return max(0, min(3, D - 1))


# ---- the oracle's side of the in-run record ----------------------------------------------------------------------------
def oracle_bytes(e, t):
    """The bits of the device's S_t byte that the fields read, from a tests/_observers.Trajectory: S_t in
    bit 0 and, for t > 1, S_{t-1} in bit 3."""
    s = np.asarray(e.S[t]).astype(np.uint8) & 1
    return s | ((np.asarray(e.S[t - 1]).astype(np.uint8) & 1) << 3) if t > 1 else s


def datasets(e, every, D, pairs, t0=1):
    """What BatchEngine.pair_map_histories holds for the replica of Trajectory e."""
    its = np.arange(t0, e.last + 1, every, dtype=np.int64)
    d = {PM.PAIR_MAP_ITERS_DATASET: its, PM.PAIR_MAP_DISTANCE_DATASET: np.int64(D)}
    fields = {int(t): PM.host_fields(oracle_bytes(e, int(t)), int(t)) for t in its}
    for a, b in pairs:
        maps = [PM.host_pair_map(fields[int(t)][a], fields[int(t)][b], D) for t in its]
        d[PM.dataset_name(a, b)] = np.array(maps, dtype=np.int64).reshape((len(its),) + PM.map_shape(D))
    return d


def compare(got, want, k):
    assert list(got) == list(want), (k, list(got), list(want))
    for name, w in want.items():
        g = np.asarray(got[name])
        assert g.dtype == np.int64 and g.shape == np.shape(w) and np.array_equal(g, w), (k, name, g.shape, np.shape(w))
