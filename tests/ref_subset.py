"""Host restatement of the surface subset (cvhip_surface_subset, csrc/subset_kernels.hip): the reference's
max_points (triangulation.rs:837-843, `tracks.shuffle(rng); tracks.truncate(max_points)` with an OS-seeded generator) on a
counter-based generator, as tests/ref_ransac_sampler.py does for the RANSAC samplers.

  key(seed, i) = mix64(mix64(seed) + (i + 1) * 0x9E3779B97F4A7C15)      all modulo 2^64

- output i of splitmix64 started at mix64(seed); mix64 is a bijection and the multiplier is odd, so the keys of one seed are
pairwise distinct.  The max_points rows with the smallest keys are kept, in ascending row order (the reference's order is
random: a defined departure).  numpy uint64 - test infrastructure, not product code."""
from __future__ import annotations

import numpy as np

from ref_ransac_sampler import GOLDEN, mix64


def keys(n, seed):
    """key(seed, i) for i = 0 .. n-1 -> [n] uint64."""
    i = np.arange(1, int(n) + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64(mix64(int(seed)) + i * GOLDEN)


def key(seed, i):
    """key(seed, i) of one row, with Python integers -> int."""
    mask = 0xFFFFFFFFFFFFFFFF
    return int(mix64((int(mix64(int(seed))) + (int(i) + 1) * int(GOLDEN)) & mask))


def key_order(k):
    """The rows in ascending (key, row) order (a stable sort: equal keys stay in row order) - shared by the selections of
    several m on the same keys."""
    return np.argsort(np.asarray(k, dtype=np.uint64).reshape(-1), kind="stable")


def select_smallest(k, m, order=None):
    """The rows of the m smallest (key, row) pairs of the uint64 keys `k` (of equal keys the lower row), ascending ->
    [min(n, m)] uint64.  order: key_order(k), when the caller has it."""
    k = np.asarray(k, dtype=np.uint64).reshape(-1)
    n, m = len(k), int(m)
    if m >= n:
        return np.arange(n, dtype=np.uint64)
    order = key_order(k) if order is None else order
    return np.sort(order[:m]).astype(np.uint64)


def subset_rows(n, max_points, seed):
    """The rows that max_points keeps of n, ascending -> [min(n, max_points)] uint64."""
    if int(max_points) >= int(n):  # the reference only acts when len > max_points
        return np.arange(int(n), dtype=np.uint64)
    return select_smallest(keys(n, seed), max_points)
