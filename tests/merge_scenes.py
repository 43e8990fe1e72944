"""Track tables for the merge_tracks tests (test_merge_tracks_ref.py, test_merge_tracks_gpu.py)."""
import math

import numpy as np

import ref_merge

# DESIGN.md 4.10's worked example: w = h = 8, two images, merged image 0; row 4's image-1 point is (x4, 4)
WORKED_SHAPE = (8, 8)


def worked_table(x4):
    t = np.full((5, 2, 2), -1, dtype=np.int32)
    t[0] = [(3, 3), (20, 3)]
    t[1] = [(3, 3), (30, 3)]
    t[2, 0] = (6, 6)
    t[3, 1] = (5, 5)
    t[4] = [(3, 4), (x4, 4)]
    return t


def random_table(rng, n, m, width, height, image_index, p_present=0.8, p_other=0.7, cells=None):
    """n rows over m images.  Image i: a point in `cells` random cells of the width x height grid (all cells by default;
    fewer cells stack more tracks in each) with probability p_present; every other image: with probability p_other, the
    image-i location (or a random one) plus an offset of up to about 0.8 d per axis, so that the distances between the
    tracks of a window fall on both sides of max_distance_sqr."""
    _, d2 = ref_merge.radius_and_distance(width, height)
    s = max(1, int(0.8 * math.isqrt(d2)))
    ncell = width * height if cells is None else min(cells, width * height)
    pool = rng.choice(width * height, size=ncell, replace=False) if ncell < width * height else None
    c = rng.integers(0, ncell, size=n)
    if pool is not None:
        c = pool[c]
    base = np.stack([c % width, c // width], axis=1).astype(np.int64)
    t = np.full((n, m, 2), -1, dtype=np.int32)
    for j in range(m):
        if j == image_index:
            on = rng.random(n) < p_present
            t[on, j] = base[on]
        else:
            on = rng.random(n) < p_other
            pts = base + 3 * s + rng.integers(-s, s + 1, size=(n, 2))
            t[on, j] = pts[on]
    return t
