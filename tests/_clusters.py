"""Shared by the cluster-labelling tests: the masks, the host expectation (scipy's labelling,
merged across the seam by this module's own union-find for the periodic mode) and a NumPy
model of the device scheme (csrc/spgg_clusters.hip): the same scan / resolve / relabel order
and the same pass cap."""
import numpy as np

DEFECTOR = 0xFFFF


# -- masks (True = cooperator) ------------------------------------------------
def serpentine(L):
    """Full rows 0, 2, 4, ... joined alternately at the right and the left end: one path."""
    m = np.zeros((L, L), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, L, 2)):
        m[y, L - 1 if k % 2 == 0 else 0] = True
    return m


def serpentines(L):
    """All four orientations: the path starts at the top, at the bottom, at the left, at the right."""
    s = serpentine(L)
    return [s, s[::-1].copy(), s.T.copy(), s.T[:, ::-1].copy()]


def spiral(L):
    """A one-cell-wide rectangular spiral from the corner inwards, walls one cell wide."""
    m = np.zeros((L, L), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    for _ in range(L * L):
        ny, nx = y + dy, x + dx
        ay, ax = y + 2 * dy, x + 2 * dx   # the cell after the next: keep a wall before the path
        if not (0 <= ny < L and 0 <= nx < L) or m[ny, nx] or (0 <= ay < L and 0 <= ax < L and m[ay, ax]):
            dy, dx = dx, -dy               # turn right
            ny, nx = y + dy, x + dx
            ay, ax = y + 2 * dy, x + 2 * dx
            if not (0 <= ny < L and 0 <= nx < L) or m[ny, nx] or (0 <= ay < L and 0 <= ax < L and m[ay, ax]):
                break
        y, x = ny, nx
        m[y, x] = True
    return m


def ring(L):
    """The lattice's frame: one ring touching all four edges (and, periodic, itself)."""
    m = np.zeros((L, L), dtype=bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    return m


def checkerboard(L):
    y, x = np.indices((L, L))
    return (y + x) % 2 == 0


def random_mask(L, p, seed):
    return np.random.RandomState(seed).rand(L, L) < p


def single_cell(L):
    m = np.zeros((L, L), dtype=bool)
    m[L // 2, L // 3] = True
    return m


def pattern_masks(L, seed=0):
    """The named masks of one side, as (name, mask) pairs."""
    out = [(f"serpentine{k}", m) for k, m in enumerate(serpentines(L))]
    out += [("spiral", spiral(L)), ("ring", ring(L)), ("checkerboard", checkerboard(L)),
            ("all_c", np.ones((L, L), dtype=bool)), ("all_d", np.zeros((L, L), dtype=bool)),
            ("single", single_cell(L))]
    out += [(f"random{p}", random_mask(L, p, seed + i)) for i, p in enumerate((0.55, 0.593, 0.7))]
    return out


# -- host expectation -------------------------------------------------------------
def expected_sizes(mask, periodic=False):
    """int64 sizes of the 4-connected clusters of `mask` in label order (ascending smallest
    raster index): scipy.ndimage.label; periodic: its labels merged across the two seams."""
    from scipy.ndimage import label
    mask = np.asarray(mask, dtype=bool)
    lab, k = label(mask)
    counts = np.bincount(lab.ravel(), minlength=k + 1).astype(np.int64)
    if not periodic:
        return counts[1:]
    parent = list(range(k + 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    pairs = list(zip(lab[0], lab[-1])) + list(zip(lab[:, 0], lab[:, -1]))
    for a, b in pairs:
        if a and b:
            ra, rb = find(int(a)), find(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)   # the smaller label (first in raster order) stays
    merged = np.zeros(k + 1, dtype=np.int64)
    for a in range(1, k + 1):
        merged[find(a)] += counts[a]
    return merged[[a for a in range(1, k + 1) if find(a) == a]]


def expected_record(S, periodic=False):
    """(n_clusters, largest, cd_bonds) of a strategy plane S (0 = cooperator)."""
    S = np.asarray(S) & 1
    sz = expected_sizes(S == 0, periodic)
    bonds = int(np.sum(S != np.roll(S, 1, 0)) + np.sum(S != np.roll(S, 1, 1)))
    return len(sz), int(sz.max()) if len(sz) else 0, bonds


# -- NumPy model of the device scheme -------------------------------------------------
def model(mask, periodic, cap):
    """(size plane (n,) int64, passes) as csrc/spgg_clusters.hip computes them, or (None, cap)
    when the pass cap is reached (the kernel's n_clusters = -1).  A pass is one scan."""
    mask = np.asarray(mask, dtype=bool)
    L = mask.shape[0]
    n = L * L
    idx = np.arange(n)
    # a cooperator starts with the index of the first cell of its row run
    start = mask & ~np.concatenate([np.zeros((L, 1), dtype=bool), mask[:, :-1]], axis=1)
    run = np.maximum.accumulate(np.where(start, idx.reshape(L, L), -1), axis=1)
    label = np.where(mask, run, DEFECTOR).ravel()
    ref = idx.copy()
    for passes in range(1, cap + 1):
        # scan: minimum label among the cooperator neighbours (a defector's label is the maximum)
        lab2 = label.reshape(L, L)
        m = lab2.copy()
        for shift, axis in ((1, 0), (-1, 0), (1, 1), (-1, 1)):
            nb = np.roll(lab2, shift, axis)
            if not periodic:   # the wrapped row / column is a wall
                edge = [slice(None), slice(None)]
                edge[axis] = 0 if shift == 1 else L - 1
                nb[tuple(edge)] = DEFECTOR
            m = np.minimum(m, nb)
        m = m.ravel()
        low = (label != DEFECTOR) & (m < label)
        if not low.any():
            coop = label != DEFECTOR
            counts = np.bincount(label[coop], minlength=n).astype(np.int64)
            return np.where(label == idx, counts, 0), passes
        np.minimum.at(ref, label[low], m[low])
        assert np.all(ref <= idx)
        # resolve: every representative whose ref was lowered follows ref to its end
        reps = np.nonzero((label == idx) & (ref != idx))[0]
        r = ref[reps]
        for _ in range(n):
            q = ref[r]
            if np.array_equal(q, r):
                break
            r = q
        label[reps] = r
        # relabel
        coop = label != DEFECTOR
        label[coop] = label[label[coop]]
    return None, cap
