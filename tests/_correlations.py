"""Shared by the pair-correlation tests: the host expectation (np.roll, written out here and not
taken from the package) and a NumPy model of the device scheme (csrc/spgg_correlations.hip):
rows packed into 32-bit words, the same cyclic rotation of an L-bit string with the same wrap
handling, the same flattened column shift."""
import numpy as np

WORD = 32   # spgg_co::kWordBits


# -- host expectation -------------------------------------------------------------
def expected_pair_counts(mask, max_d):
    """int64 (2, max_d + 1): [0, d] = sum(c & roll(c, -d, axis=1)), [1, d] = sum(c & roll(c, -d, axis=0))."""
    c = np.asarray(mask, dtype=bool)
    out = np.zeros((2, max_d + 1), dtype=np.int64)
    for d in range(max_d + 1):
        out[0, d] = int(np.sum(c & np.roll(c, -d, axis=1)))
        out[1, d] = int(np.sum(c & np.roll(c, -d, axis=0)))
    return out


# -- NumPy model of the device scheme ------------------------------------------------
def row_words(L):
    return (L + WORD - 1) // WORD


def pack(mask):
    """uint32 (L, W): cell x of a row at bit x & 31 of word x >> 5, bits >= L zero."""
    c = np.asarray(mask, dtype=bool)
    L, W = c.shape[0], row_words(c.shape[0])
    padded = np.zeros((L, W * WORD), dtype=np.uint64)
    padded[:, :L] = c
    weights = np.uint64(1) << np.arange(WORD, dtype=np.uint64)
    return (padded.reshape(L, W, WORD) * weights).sum(axis=2).astype(np.uint32)


def unpack(words, L):
    words = np.asarray(words, dtype=np.uint32)
    b = (words[:, :, None] >> np.arange(WORD, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(words.shape[0], -1)[:, :L].astype(bool)


def rotated_word(row, w, d, L):
    """Word w of the row rotated by d as the kernel builds it: 32 bits from bit s = (32 w + d) mod L
    of the L-bit cyclic string (two words funnelled; the word after the last reads as 0), and where
    fewer than 32 bits are left before the wrap, word 0 shifted up behind them."""
    W = row_words(L)
    s = WORD * w + d
    assert s < 2 * L
    if s >= L:
        s -= L
    a, sh = s >> 5, s & 31
    lo = int(row[a])
    hi = int(row[a + 1]) if a + 1 < W else 0
    v = (((hi << 32) | lo) >> sh) & 0xFFFFFFFF
    k = L - s
    assert k >= 1
    if k < WORD:
        v = ((v & ((1 << k) - 1)) | (int(row[0]) << k)) & 0xFFFFFFFF
    return v


def model_rotate(mask, d):
    """roll(mask, -d, axis=1) through the packed rotation; the bits of a word beyond the row's
    cells are arbitrary in the kernel (they meet zero padding) and are cut here."""
    c = np.asarray(mask, dtype=bool)
    L, W = c.shape[0], row_words(c.shape[0])
    words = pack(c)
    rot = np.array([[rotated_word(words[y], w, d, L) for w in range(W)] for y in range(L)], dtype=np.uint32)
    return unpack(rot, L)


def _popcount(a):
    a = np.asarray(a, dtype=np.uint32)
    return int(np.unpackbits(a.view(np.uint8)).sum())


def model_pair_counts(mask, max_d):
    """The kernel's counts: AND + popcount of packed words, the column partner found by the
    flattened shift (i + d W) mod L W."""
    c = np.asarray(mask, dtype=bool)
    L, W = c.shape[0], row_words(c.shape[0])
    words = pack(c)
    flat = words.ravel()
    out = np.zeros((2, max_d + 1), dtype=np.int64)
    for d in range(max_d + 1):
        rot = np.array([[rotated_word(words[y], w, d, L) for w in range(W)] for y in range(L)], dtype=np.uint32)
        out[0, d] = _popcount(words & rot)
        j = np.arange(L * W) + d * W
        j = np.where(j >= L * W, j - L * W, j)
        out[1, d] = _popcount(flat & flat[j])
    return out


# -- masks and planes -------------------------------------------------------------
def pattern_masks(L, seed=0):
    """(name, cooperator mask) pairs of one side."""
    y, x = np.indices((L, L))
    single = np.zeros((L, L), dtype=bool)
    single[L - 1, L - 1] = True
    cross = np.zeros((L, L), dtype=bool)
    cross[L // 2] = True
    cross[:, L // 3] = True
    rs = np.random.RandomState(1000 + 7 * L + seed)
    return [("all_c", np.ones((L, L), dtype=bool)), ("all_d", np.zeros((L, L), dtype=bool)),
            ("checkerboard", (y + x) % 2 == 0), ("single_last", single), ("row_and_column", cross),
            ("stripes3", np.broadcast_to(x % 3 == 0, (L, L)).copy()), ("random0.1", rs.rand(L, L) < 0.1)]


def planes_of(L, seed=0):
    """(names, uint8 S planes): the pattern masks as strategies (0 = cooperator), and a random
    p = 0.5 plane with random bookkeeping bits 1-4 set (only bit 0 counts)."""
    masks = pattern_masks(L, seed)
    names = [n for n, _ in masks] + ["random0.5_dirty_bits"]
    planes = [np.where(m, 0, 1).astype(np.uint8) for _, m in masks]
    rs = np.random.RandomState(2000 + 11 * L + seed)
    planes.append((np.where(rs.rand(L, L) < 0.5, 0, 1) | (rs.randint(0, 16, (L, L)) << 1)).astype(np.uint8))
    return names, planes
