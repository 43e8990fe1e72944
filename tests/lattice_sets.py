"""Integer point sets for the lattice path of cvhip_mesh_delaunay, shared by tests/test_delaunay_lattice_cpu.py
and tests/test_delaunay_lattice_gpu.py, and the affine surfaces over them."""
import numpy as np

import ref_delaunay as rd

SCALE = float(2 ** 20)
LIMIT = float(2 ** 24)  # LatticePolicy's bound on |coordinate|


def holes(nx, ny, seed, share=0.10):
    """the nx x ny integer lattice, row-major, without a seeded `share` of its points"""
    xy = rd.lattice(nx, ny)
    return np.ascontiguousarray(xy[np.random.default_rng(seed).random(len(xy)) >= share])


def circle50_lowest_at(position):
    """circle50 with index 0 exchanged with the index at `position`: the tie polygon's lowest index sits somewhere else"""
    xy = rd.circle50().copy()
    xy[[0, position]] = xy[[position, 0]]
    return xy


def circle50_near_tie():
    """circle50 scaled by 2^20 with one of the 12 co-circular points moved by 1: a tie no more, by one part in 2^23 of the
    radius (with |coordinates| <= 2^24 a determinant that is not zero stays far above the f64 filter's bound - measured: 2.8e19
    against 1.5e12 here - so this pins the filter-first order; the integers decide the exact zeros next to it)"""
    xy = rd.circle50() * SCALE
    on = np.flatnonzero((rd.circle50() ** 2).sum(axis=1) == 50.0)
    xy[on[3], 0] += 1.0
    return xy


def with_duplicates(seed=21):
    """a 24 x 20 lattice with holes, 40 of its points repeated (5 of them three times), shuffled -> (xy, number of duplicates)"""
    rng = np.random.default_rng(seed)
    base = holes(24, 20, seed)
    xy = np.concatenate([base, base[:40], base[10:15]])
    return np.ascontiguousarray(xy[rng.permutation(len(xy))]), 45


SETS = {
    "lattice_17x13": rd.lattice,
    "holes_96": lambda: holes(96, 96, 96),
    "circle50_a": lambda: circle50_lowest_at(3), "circle50_b": lambda: circle50_lowest_at(7), "circle50_c": lambda: circle50_lowest_at(13),
    "scaled_16x16": lambda: rd.lattice(16, 16) * SCALE,          # differences up to 15 * 2^20: the in-circle products need ~2^81
    "near_tie": circle50_near_tie,
    "offset": lambda: holes(20, 15, 3) + (LIMIT - 100.0),        # coordinates up to 2^24 - 81
    "negative": lambda: -holes(15, 20, 4) - np.array([3.0, 0.0]),
    "mixed_sign": lambda: holes(21, 17, 5) * np.array([1677721.0, 1.0]) - np.array([LIMIT, 8.0]),  # x from -2^24 to 2^24 - 12
}


def affine_points(nx, ny, seed, share=0.10):
    """(points3d [n, 3], p2 [n, 2]) as triangulate_affine returns them: the pixels of an nx x ny image that found a match, in scan
    order, with a smooth non-negative depth"""
    xy = holes(nx, ny, seed, share)
    z = 6.0 + 3.0 * np.sin(xy[:, 0] / 7.0) * np.cos(xy[:, 1] / 5.0) + 0.01 * xy[:, 0]
    p2 = np.stack([xy[:, 0] + np.floor(z), xy[:, 1]], axis=1).astype(np.uint32)
    return np.concatenate([xy, z[:, None]], axis=1), p2
