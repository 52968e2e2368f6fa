"""The labelling scheme of csrc/spgg_clusters.hip as a NumPy model (tests/_clusters.py: the same
scan / resolve / relabel order, the same pass cap) against scipy.ndimage.label: sizes, label
order, both boundary modes -- and the pass counts the kernel's cap is taken from.

The cap (SPGG_CLUSTERS_MAX_PASSES in include/spgg_abi.h, _lib.CLUSTERS_MAX_PASSES) must be at
least four times the largest pass count the model needs over the masks below at the supported
side; DESIGN.md section 8 quotes the observed maximum."""
import os
import re

import numpy as np
import pytest

pytest.importorskip("scipy")

from spgg_amd import _lib  # noqa: E402

from tests import _clusters as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = _lib.CLUSTERS_MAX_PASSES
SIDE = 200   # spgg_clusters_max_side (csrc/spgg_clusters.h kMaxSide)
OBSERVED_MAX_PASSES = 5   # over both boundary modes at SIDE; DESIGN.md section 8 quotes it


def _check(mask, periodic):
    plane, passes = K.model(mask, periodic, CAP)
    assert plane is not None, "pass cap reached"
    want = K.expected_sizes(mask, periodic)
    got = plane[plane > 0]
    assert np.array_equal(got, want), (got[:8], want[:8])
    # a representative is the smallest raster index of its cluster: non-periodic, scipy's
    # label k first appears (raster order) exactly there
    if not periodic and len(want):
        from scipy.ndimage import label
        lab = label(mask)[0].ravel()
        first = np.array([np.argmax(lab == k) for k in range(1, min(len(want), 50) + 1)])
        assert np.array_equal(np.nonzero(plane)[0][:len(first)], first)
    return passes


def test_constants_agree_with_the_sources():
    hdr = open(os.path.join(ROOT, "include", "spgg_abi.h")).read()
    assert int(re.search(r"#define SPGG_CLUSTERS_MAX_PASSES (\d+)", hdr).group(1)) == CAP
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    src = open(os.path.join(pkg, "csrc", "spgg_clusters.h")).read()
    assert int(re.search(r"kMaxSide = (\d+);", src).group(1)) == SIDE
    assert "kMaxPasses = SPGG_CLUSTERS_MAX_PASSES;" in src


@pytest.mark.parametrize("L", [1, 2, 3, 5, 13, 33])
@pytest.mark.parametrize("periodic", [False, True])
def test_random_masks_small_sides(L, periodic):
    for seed in range(12):
        for p in (0.3, 0.55, 0.593, 0.7, 0.9):
            _check(K.random_mask(L, p, 1000 * seed + int(p * 100)), periodic)
    for _name, m in K.pattern_masks(L):
        _check(m, periodic)


def test_supported_side_patterns_and_pass_cap():
    worst = {}
    for periodic in (False, True):
        for name, m in K.pattern_masks(SIDE):
            if name == "single":
                continue
            worst[(name, periodic)] = _check(m, periodic)
    print(sorted(worst.items(), key=lambda kv: -kv[1])[:6])
    top = max(worst.values())
    assert top == OBSERVED_MAX_PASSES, worst   # (the figure DESIGN.md quotes)
    assert 4 * top <= CAP, (top, CAP)


def test_cap_is_reported():
    """The cap itself: a mask needing more passes than allowed gives no sizes (the kernel's
    n_clusters = -1), never a wrong answer."""
    m = K.random_mask(33, 0.593, 5)
    _plane, need = K.model(m, False, CAP)
    assert need >= 3
    assert K.model(m, False, need - 1)[0] is None
