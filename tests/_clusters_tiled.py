"""NumPy model of the tiled device labelling (csrc/spgg_clusters_tiled.hip), shared by its tests:
tile-local labels with the tile edge as a wall (the scan / resolve / relabel passes of
tests/_clusters.model on a rectangle), seam unions that link the larger root under the smaller
with a minimum and retry from the value seen, root walks with path halving, per-root counts and
the three-value record.

Concurrency is modelled in lock step, the way a GPU runs it: every walker of a launch takes its
step at the same time on the live parent plane, and every union of a seam pass looks for its two
roots before any of them links (so unions do lose their minimum and retry, as on the device).
The model reports the most passes a tile needed, the longest root walk and the most retries of a
union; the device caps are held against them."""
import numpy as np

from tests import _clusters as K

DEFECTOR = K.DEFECTOR
TILE_MIN, TILE_MAX = 8, 200


def tile_labels(mask, cap):
    """(local labels (h*w,), passes) of one h x w tile with its edge as a wall, labels the local
    raster index of the tile cluster's first cell (DEFECTOR for a defector); (None, cap) on the
    pass cap."""
    h, w = mask.shape
    m = h * w
    idx = np.arange(m)
    start = mask & ~np.concatenate([np.zeros((h, 1), dtype=bool), mask[:, :-1]], axis=1)
    run = np.maximum.accumulate(np.where(start, idx.reshape(h, w), -1), axis=1)
    label = np.where(mask, run, DEFECTOR).ravel()
    ref = idx.copy()
    for passes in range(1, cap + 1):
        lab2 = label.reshape(h, w)
        mn = lab2.copy()
        mn[1:] = np.minimum(mn[1:], lab2[:-1])
        mn[:-1] = np.minimum(mn[:-1], lab2[1:])
        mn[:, 1:] = np.minimum(mn[:, 1:], lab2[:, :-1])
        mn[:, :-1] = np.minimum(mn[:, :-1], lab2[:, 1:])
        mn = mn.ravel()
        low = (label != DEFECTOR) & (mn < label)
        if not low.any():
            return label, passes
        np.minimum.at(ref, label[low], mn[low])
        assert np.all(ref <= idx)
        reps = np.nonzero((label == idx) & (ref != idx))[0]
        r = ref[reps]
        for _ in range(m):
            q = ref[r]
            if np.array_equal(q, r):
                break
            r = q
        label[reps] = r
        coop = label != DEFECTOR
        label[coop] = label[label[coop]]
    return None, cap


def find_roots(parent, x):
    """(roots, most loop iterations of one walker) of lock-step walks from the cells x with path
    halving on the live plane: an iteration reads p = parent[x] and gp = parent[p], ends at a root
    (p == x or gp == p) or lowers parent[x] to gp and goes on from gp."""
    x = np.array(x, dtype=np.int64)
    root = np.empty_like(x)
    active = np.arange(x.size)
    iters = 0
    while active.size:
        iters += 1
        xa = x[active]
        p = parent[xa]
        gp = parent[p]
        assert np.all(p <= xa) and np.all(gp <= p)
        end = (p == xa) | (gp == p)
        root[active[end]] = p[end]
        go = ~end
        np.minimum.at(parent, xa[go], gp[go])
        x[active[go]] = gp[go]
        active = active[go]
    return root, iters


def seam_pairs(L, tile, periodic):
    """The (a, b) raster indices of the cells facing each other across the tile edges, in the
    device's order: between tile columns, then between tile rows; the lattice edge last."""
    ntx = -(-L // tile)
    cuts = [((s + 1) * tile - 1, (s + 1) * tile) for s in range(ntx - 1)] + ([(L - 1, 0)] if periodic else [])
    along = np.arange(L)
    a = [along * L + ca for ca, _ in cuts] + [ca * L + along for ca, _ in cuts]
    b = [along * L + cb for _, cb in cuts] + [cb * L + along for _, cb in cuts]
    if not cuts:
        return np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)
    return np.concatenate(a), np.concatenate(b)


def model(mask, periodic, tile, pass_cap=32):
    """(size plane (n,) int64, (clusters, largest, bonds), stats) as spgg_clusters_tiled computes
    them; stats = dict(passes, walk, retries): the most passes of a tile, the most iterations of a
    root walk and the most retries of a union."""
    mask = np.asarray(mask, dtype=bool)
    L = mask.shape[0]
    n = L * L
    tile = min(tile, L)
    idx = np.arange(n)
    parent = idx.copy()
    stats = dict(passes=0, walk=0, retries=0)
    # tile pass
    for y0 in range(0, L, tile):
        for x0 in range(0, L, tile):
            sub = mask[y0:y0 + tile, x0:x0 + tile]
            h, w = sub.shape
            lab, passes = tile_labels(sub, pass_cap)
            assert lab is not None, "pass cap"
            stats["passes"] = max(stats["passes"], passes)
            coop = lab != DEFECTOR
            ry, rx = np.divmod(np.where(coop, lab, 0), w)
            g = ((y0 + np.arange(h))[:, None] * L + x0 + np.arange(w)[None, :]).ravel()
            parent[g[coop]] = ((y0 + ry) * L + x0 + rx)[coop]
    assert np.all(parent <= idx)
    # seam pass: every pending union finds its roots, then the minima are applied one by one
    a, b = seam_pairs(L, tile, periodic)
    keep = (a != b) & mask.ravel()[a] & mask.ravel()[b]
    a, b = a[keep], b[keep]
    rounds = 0
    while a.size:
        ra, it_a = find_roots(parent, a)
        rb, it_b = find_roots(parent, b)
        stats["walk"] = max(stats["walk"], it_a, it_b)
        hi, lo = np.maximum(ra, rb), np.minimum(ra, rb)
        na, nb = [], []
        for h_, l_ in zip(hi.tolist(), lo.tolist()):
            if h_ == l_:
                continue
            old = parent[h_]
            parent[h_] = min(old, l_)   # the atomic minimum, returning old
            if old != h_:               # lost: hi had been linked first; (old, lo) are still to be united
                assert old < h_
                na.append(old)
                nb.append(l_)
        if na:
            rounds += 1
        a, b = np.array(na, dtype=np.int64), np.array(nb, dtype=np.int64)
    stats["retries"] = rounds
    # count
    cells = idx[mask.ravel()]
    root, it = find_roots(parent, cells)
    stats["walk"] = max(stats["walk"], it)
    count = np.bincount(root, minlength=n).astype(np.int64)
    # record
    is_root = mask.ravel() & (parent == idx)
    sizes = np.where(is_root, count, 0)
    S = (~mask).astype(np.int64)
    bonds = int(np.sum(S != np.roll(S, 1, 0)) + np.sum(S != np.roll(S, 1, 1)))
    rec = (int(is_root.sum()), int(sizes.max()) if n else 0, bonds)
    return sizes, rec, stats

