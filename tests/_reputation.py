"""Shared by the reputation-record tests: the host expectations (np.roll and np.histogram, written
out here and not taken from the package) and a NumPy model of the device schemes
(csrc/spgg_reputation.hip): rows padded to dwords of four int8 cells, the shifted dword built from
two aligned ones with one wrap per row, the flattened column shift, the dot of four int8 products,
and the bisection that bins a value among ascending edges."""
import numpy as np

CELLS = 4            # spgg_rp::kCellsPerDword
DOT_MAX = 4 * 128 * 128   # spgg_rp::kDotMax
SMALL_DWORDS = 65536 // 4    # spgg_rp::kSmallDwords
FULL_DWORDS = 163840 // 4    # spgg_rp::kFullDwords
WAVES = 16           # spgg_rp::kWaves


# -- host expectation -------------------------------------------------------------
def expected_pair_sums(K, max_d):
    """(sum, rows, cols) int64 by the definition: rows[d] = sum(K * roll(K, -d, axis=1)),
    cols[d] = sum(K * roll(K, -d, axis=0))."""
    K = np.asarray(K).astype(np.int64)
    rows, cols = np.zeros(max_d + 1, dtype=np.int64), np.zeros(max_d + 1, dtype=np.int64)
    for d in range(max_d + 1):
        rows[d] = int(np.sum(K * np.roll(K, -d, axis=1)))
        cols[d] = int(np.sum(K * np.roll(K, -d, axis=0)))
    return int(K.sum()), rows, cols


def loop_pair_sums(K, max_d):
    """The same by a direct double loop over the cells (small lattices only)."""
    K = np.asarray(K)
    L = K.shape[0]
    rows, cols = [0] * (max_d + 1), [0] * (max_d + 1)
    total = 0
    for y in range(L):
        for x in range(L):
            total += int(K[y][x])
            for d in range(max_d + 1):
                rows[d] += int(K[y][x]) * int(K[y][(x + d) % L])
                cols[d] += int(K[y][x]) * int(K[(y + d) % L][x])
    return total, np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64)


def expected_hist(S, X, bins, lo, hi):
    """int64 (2, bins): np.histogram of the cooperators' (bit 0 of S clear) and of the defectors'
    values over range (lo, hi)."""
    S, X = np.asarray(S), np.asarray(X, dtype=np.float64)
    coop = (S.astype(np.int64) & 1) == 0
    return np.stack([np.histogram(X[coop], bins=bins, range=(lo, hi))[0],
                     np.histogram(X[~coop], bins=bins, range=(lo, hi))[0]]).astype(np.int64)


def edges_of(lo, hi, bins):
    return np.histogram_bin_edges(np.empty(0), bins, (float(lo), float(hi)))


# -- fields ------------------------------------------------------------------------
FIELD_NAMES = ("all_min", "all_max", "checkerboard", "single_cell", "x_ramp", "y_ramp", "random")


def fields_of(L, seed=0):
    """The int8 (L, L) test fields, in FIELD_NAMES' order: the two extreme magnitudes, a +-127/-128
    checkerboard, one non-zero cell, ramps over the whole int8 range along x and along y, and
    uniform random bytes."""
    rs = np.random.RandomState(1000 + 7 * L + seed)
    y, x = np.mgrid[0:L, 0:L]
    single = np.zeros((L, L), dtype=np.int64)
    single[L // 3, (2 * L) // 3] = -128
    ramp = lambda v: ((v * 37) % 256) - 128   # every level at L >= 256, spread over the range below
    out = [np.full((L, L), -128), np.full((L, L), 127), np.where((x + y) & 1, 127, -128), single,
           ramp(x), ramp(y), rs.randint(-128, 128, (L, L))]
    return [f.astype(np.int8) for f in out]


def strategy_planes(L, count, seed=0):
    """uint8 S planes for `count` replicas: random strategies, the last with dirty bookkeeping bits
    (bits 1-4), which no count may depend on."""
    rs = np.random.RandomState(2000 + L + seed)
    planes = [rs.randint(0, 2, (L, L)).astype(np.uint8) for _ in range(count)]
    planes[-1] = (planes[-1] | (rs.randint(0, 16, (L, L)) << 1)).astype(np.uint8)
    return planes


# -- NumPy model of the pair-sum scheme ----------------------------------------------
def row_dwords(L):
    return (L + CELLS - 1) // CELLS


def pad(K):
    """uint32 (L, W): cell x of a row at byte x & 3 of dword x >> 2, the bytes >= L zero."""
    K = np.asarray(K, dtype=np.int8)
    L, W = K.shape[0], row_dwords(K.shape[0])
    b = np.zeros((L, W * CELLS), dtype=np.uint8)
    b[:, :L] = K.view(np.uint8)
    return b.view("<u4").reshape(L, W)


def dot4(a, b):
    """The int8 dot instruction on dwords (arrays): sum of the four signed byte products, int64."""
    a = np.ascontiguousarray(np.asarray(a, dtype="<u4")).view(np.int8).reshape(-1, CELLS).astype(np.int64)
    b = np.ascontiguousarray(np.asarray(b, dtype="<u4")).view(np.int8).reshape(-1, CELLS).astype(np.int64)
    out = (a * b).sum(axis=1)
    assert np.all(np.abs(out) <= DOT_MAX)
    return out


def rotated_dwords(lat, d, L):
    """uint32 (L, W): dword w of every row rotated by d as the kernel builds it: 4 bytes from byte
    s = (4 w + d) mod L of the L-byte cyclic string (two aligned dwords through alignbyte; the dword
    after the last reads as 0), and where k = L - s < 4 bytes are left before the wrap, dword 0
    shifted up by k bytes behind them."""
    W = row_dwords(L)
    lat = np.asarray(lat, dtype=np.uint64)
    out = np.zeros((L, W), dtype=np.uint64)
    zero = np.zeros(L, dtype=np.uint64)
    for w in range(W):
        s = CELLS * w + d
        assert s < 2 * L
        if s >= L:
            s -= L
        a, sh = s >> 2, s & 3
        lo = lat[:, a]
        hi = lat[:, a + 1] if a + 1 < W else zero
        v = (((hi << np.uint64(32)) | lo) >> np.uint64(8 * sh)) & np.uint64(0xFFFFFFFF)   # v_alignbyte_b32
        k = L - s
        assert k >= 1
        if k < CELLS:
            v = ((v & np.uint64((1 << (8 * k)) - 1)) | (lat[:, 0] << np.uint64(8 * k))) & np.uint64(0xFFFFFFFF)
        out[:, w] = v
    return out.astype(np.uint32)


def model_rotate(K, d):
    """The valid cells of the rotated row, as int8 (L, L): equals np.roll(K, -d, axis=1)."""
    L = np.asarray(K).shape[0]
    rot = rotated_dwords(pad(K), d, L)
    return np.ascontiguousarray(rot.astype("<u4")).view(np.int8).reshape(L, -1)[:, :L]


def model_pair_sums(K, max_d):
    """(sum, rows, cols) the way the LDS instances compute them: dots over the padded dwords (the
    rotated dword's bytes beyond the row meet zero padding), lane partials of a 64-lane wave held
    to int32, reduced in int64."""
    L = np.asarray(K).shape[0]
    W = row_dwords(L)
    lat = pad(K)
    flat = lat.reshape(-1)
    lanes = np.arange(flat.size) % 64   # dword i is lane i & 63's in the column sweep

    def reduce(dots):
        part = np.zeros(64, dtype=np.int64)
        np.add.at(part, lanes, dots)
        assert np.all(np.abs(part) < 2 ** 31)
        return int(part.sum())

    ones = np.full(flat.size, 0x01010101, dtype=np.uint32)
    total = reduce(dot4(flat, ones))
    rows, cols = np.zeros(max_d + 1, dtype=np.int64), np.zeros(max_d + 1, dtype=np.int64)
    for d in range(max_d + 1):
        rows[d] = reduce(dot4(flat, rotated_dwords(lat, d, L).reshape(-1)))
        j = (np.arange(flat.size) + d * W) % flat.size
        cols[d] = reduce(dot4(flat, flat[j]))
    return total, rows, cols


# -- model of the bin rule --------------------------------------------------------------
def model_bin(edges, x):
    """The kernel's bin of x among ascending edges: bisect for the number of edges <= x (9 halvings
    cover 257 edges); -1 if x lies outside, the last bin if x is the last edge."""
    bins = len(edges) - 1
    lo, hi = 0, bins + 1
    for _ in range(9):
        if lo < hi:
            mid = (lo + hi) >> 1
            if edges[mid] <= x:
                lo = mid + 1
            else:
                hi = mid
    assert lo == hi
    if lo == 0:
        return -1
    if lo == bins + 1:
        return bins - 1 if x == edges[bins] else -1
    return lo - 1


def model_hist(edges, values):
    out = np.zeros(len(edges) - 1, dtype=np.int64)
    for x in values:
        b = model_bin(edges, x)
        if b >= 0:
            out[b] += 1
    return out
