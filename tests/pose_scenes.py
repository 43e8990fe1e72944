"""Synthetic scenes for the pose-recovery tests: config 5's cameras (synth.sfm_cameras) looking at random points, and
rigs of 2 to 8 cameras with ragged tracks, planted matches per pair and the special scenes of the multi-view tests (what
each one is for is shown on the CPU by tests/test_pose_ref.py)."""
import numpy as np

import mixed_scenes
from cybervision_amd import synth


def scene(n=3000, size=512, seed=3, noise=True):
    """-> (tracks [n, 3, 2] int32, K, poses, X [n, 3]): points in front of all three cameras, projected and rounded."""
    K, poses = synth.sfm_cameras(size)
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(40, size - 40, size=(n, 2))
    z = rng.uniform(0.8, 1.2, size=n)
    X = (np.linalg.inv(K) @ np.stack([p0[:, 0], p0[:, 1], np.ones(n)])).T * z[:, None]
    tracks = np.zeros((n, 3, 2), dtype=np.int32)
    for j, (R, t) in enumerate(poses):
        q = (K @ (R @ X.T + t[:, None])).T
        px = q[:, :2] / q[:, 2:3]
        tracks[:, j] = np.rint(px).astype(np.int32) if noise else px.astype(np.int32)
    return tracks, K, poses, X


def projection(K, R, t):
    return K @ np.hstack([R, np.asarray(t, dtype=np.float64)[:, None]])


# ---- more than three views ---------------------------------------------------------------------------------------------
def rig(m, size=512):
    """K (config 5's) and m poses: camera 0 at the origin, the others translated sideways by up to 0.06 (alternating
    sides, so that neighbours in index are not neighbours in space) with rotations below 0.002 rad."""
    assert 2 <= m <= 8
    K, _ = synth.sfm_cameras(size)
    poses = [(np.eye(3), np.zeros(3))]
    for j in range(1, m):
        side = -1.0 if j % 2 else 1.0
        t = np.array([side * 0.015 * ((j + 1) // 2), 0.002 * np.sin(j), 0.001 * np.cos(2 * j)])
        poses.append((synth._rot(0.0005 * np.sin(3 * j), -0.0010 * np.cos(j), 0.0004 * np.sin(2 * j + 1)), t))
    return K, poses


def multiview_scene(m, n, size=512, seed=3, miss=0.25, bad_image=None, visible=None, spaced=False):
    """-> (tracks [n, m, 2] int32, K, poses, X [n, 3]): random points at depth 0.8..1.2 in front of rig(m), projected and
    rounded to integer pixels inside the image; every (track, view) entry is dropped with probability `miss` (ragged
    tracks), or kept where `visible` [n, m] bool says so; the points of `bad_image` are replaced by random pixels.
    spaced: the points of image 0 lie on a jittered grid, at least 13 pixels apart for n <= 400; the views' disparities
    differ by less than 6 pixels between depths, so in every image the points stay further apart than extend_tracks'
    search radius of 3 and a table built from planted matches merges no two of them."""
    K, poses = rig(m, size)
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(40, size - 40, size=(n, 2))
    if spaced:
        g = int(np.ceil(np.sqrt(n)))
        step = (size - 80) / g
        cell = rng.permutation(g * g)[:n]
        p0 = 40 + (np.stack([cell % g, cell // g], axis=1) + 0.5) * step + rng.uniform(-4, 4, size=(n, 2))
    z = rng.uniform(0.8, 1.2, size=n)
    X = (np.linalg.inv(K) @ np.stack([p0[:, 0], p0[:, 1], np.ones(n)])).T * z[:, None]
    tracks = np.zeros((n, m, 2), dtype=np.int32)
    for j, (R, t) in enumerate(poses):
        q = (K @ (R @ X.T + t[:, None])).T
        tracks[:, j] = np.rint(q[:, :2] / q[:, 2:3]).astype(np.int32)
    assert tracks.min() >= 0 and tracks.max() < size
    drop = rng.random((n, m)) < miss  # (drawn in every case, so that `visible` does not shift the later draws)
    scramble = rng.integers(0, size, size=(n, 2))
    if bad_image is not None:
        tracks[:, bad_image] = scramble
    tracks[~np.asarray(visible, dtype=bool) if visible is not None else drop] = -1
    return tracks, K, poses, X


def _k(K, j):
    """K of image j: K itself, or K[j] of a list with one K per image."""
    return K if isinstance(K, np.ndarray) and K.ndim == 2 else K[j]


def planted_matches(tracks, K, poses):
    """-> {(i, j): (matches [k, 4] uint32 (x1, y1, x2, y2), F)} for every pair i < j: the tracks seen in both images, in
    table order, and the true fundamental matrix (synth.sfm_true_f; mixed_scenes.true_f where K is a list with one K per
    image).  A pair without a common track is left out, as the
    driver leaves out a pair whose RANSAC found no F: all four candidates of its find_projection_matrix would tie at 0, and
    a tie between them follows the SVD's sign choices, which cvhip.h leaves unpinned."""
    m = tracks.shape[1]
    out = {}
    for i in range(m):
        for j in range(i + 1, m):
            both = (tracks[:, i, 0] >= 0) & (tracks[:, j, 0] >= 0)
            if not both.any():
                continue
            rows = np.concatenate([tracks[both, i], tracks[both, j]], axis=1).astype(np.uint32)
            F = synth.sfm_true_f(K, poses[i], poses[j]) if _k(K, 0) is K else \
                mixed_scenes.true_f(K[i], K[j], poses[i], poses[j])
            out[(i, j)] = (np.ascontiguousarray(rows), F)
    return out


def known_views(K, poses, placed):
    """-> (P [m, 3, 4] with zeros where unknown, has [m] uint8) for the images in `placed`; K: one matrix, or one per image."""
    m = len(poses)
    P = np.zeros((m, 3, 4))
    has = np.zeros(m, dtype=np.uint8)
    for j in placed:
        P[j] = projection(_k(K, j), *poses[j])
        has[j] = 1
    return np.ascontiguousarray(P), has


# ---- a K per image, images of different shapes ---------------------------------------------------------------------------
def mixed_multiview_scene(m, n, seed=3, miss=0.25, spaced=False, sizes=None, nested=False):
    """multiview_scene over rig(m)'s poses with mixed_scenes' cameras -> (tracks [n, m, 2] int32, Ks [m], poses, X, sizes):
    image j has its own K and its own (width, height) - mixed_scenes.dims(m, 4), 225 to 512 pixels, unless `sizes` is
    given.  The points lie where every image sees them: at depth 0.8..1.2 on rays through the box of normalised
    coordinates common to all cameras, and every pixel is inside its own image.  nested: every pixel also lies inside every
    image of a LOWER index: extend_tracks clears a merged match at its image-2 coordinates in the image-1-sized grid
    (triangulation.rs:1391-1393), and the reference panics where that is out of bounds.  spaced: the rays on a jittered
    grid, for the tables built from planted matches."""
    sizes = mixed_scenes.dims(m, 4) if sizes is None else [tuple(s) for s in sizes]
    boxes = [(min(w for w, _ in sizes[:j + 1]), min(h for _, h in sizes[:j + 1])) for j in range(m)] if nested else sizes
    Ks = mixed_scenes.calibrations(sizes)
    _, poses = rig(m)
    rng = np.random.default_rng(seed)
    x_lo, x_hi, y_lo, y_hi = mixed_scenes.common_view(Ks, boxes, 0.1 if spaced else 0.0)
    if spaced:
        g = int(np.ceil(np.sqrt(n)))
        cell = rng.permutation(g * g)[:n]
        u = (np.stack([cell % g, cell // g], axis=1) + 0.5 + rng.uniform(-0.2, 0.2, size=(n, 2))) / g
        k = n
    else:
        k = 8 * n
        u = rng.uniform(0.0, 1.0, size=(k, 2))
    z = rng.uniform(0.8, 1.2, size=k)
    X = np.stack([x_lo + u[:, 0] * (x_hi - x_lo), y_lo + u[:, 1] * (y_hi - y_lo), np.ones(k)], axis=1) * z[:, None]
    px = []
    for K, (R, t) in zip(Ks, poses):
        q = (K @ (R @ X.T + t[:, None])).T
        px.append(np.rint(q[:, :2] / q[:, 2:3]))
    px = np.stack(px, axis=1)
    inside = np.all((px >= 0) & (px < np.array(boxes, dtype=np.float64)[None]), axis=(1, 2))
    if not spaced:  # (the box is the cameras' common view up to their displacements: the first n rays inside every image)
        assert inside.sum() >= n
        X, px = X[inside][:n], px[inside][:n]
    else:
        assert inside.all()
    tracks = px.astype(np.int32)
    tracks[rng.random((n, m)) < miss] = -1
    return tracks, Ks, poses, X, sizes


# The sparse driver's mixed scene: four images, only image 2 with a side past 1000 pixels, so that extend_tracks' search
# radius (3 max_dimension / 1000 above 1000, else 3: triangulation.rs:1346-1350) is 4 for the pairs (0, 2) and (1, 2) and 3
# for every other pair; landscape and portrait; every image-2 pixel inside the smaller images before it.
SPARSE_MIXED_SIZES = [(960, 720), (720, 960), (1400, 1000), (800, 600)]


def sparse_mixed_scene(n=150, seed=12, planted=12):
    """-> (tracks, Ks, poses, X, matches, sizes): spaced points over SPARSE_MIXED_SIZES (at least 10 pixels apart in every
    image), ragged (miss 0.25), and the planted matches with the two-K F of every pair.  The first `planted` tracks A are
    seen everywhere but in image 2 (even rows) or 3 (odd rows), and each gets a companion B, appended after the others:
    seen in image 0, exactly 4 pixels left of or above A there, and in the image A misses.  extend_tracks' window is
    [p - radius, p + radius): in the pair (0, 2), radius 4, A takes B's match (B starts a track all the same); in the pair (0, 3),
    radius 3, it does not - so a radius taken from the wrong image's size changes the table."""
    full, Ks, poses, X, sizes = mixed_multiview_scene(4, n, seed=seed, miss=0.0, spaced=True, sizes=SPARSE_MIXED_SIZES,
                                                      nested=True)
    rng = np.random.default_rng(seed + 1000)
    tracks = full.copy()
    tracks[rng.random((n, 4)) < 0.25] = -1
    k0_inv = np.linalg.inv(Ks[0])
    extra, extra_x = [], []
    for k in range(planted):
        other = 2 if k % 2 == 0 else 3
        tracks[k] = full[k]
        tracks[k, other] = -1
        b = np.full((4, 2), -1, dtype=np.int32)
        b[0] = full[k, 0] + ((-4, 0) if k % 4 < 2 else (0, -4))
        xb = k0_inv @ np.array([b[0, 0], b[0, 1], 1.0]) * X[k, 2]  # (camera 0 is [I | 0]: the ray through B's pixel, at A's depth)
        R, t = poses[other]
        q = Ks[other] @ (R @ xb + t)
        b[other] = np.rint(q[:2] / q[2]).astype(np.int32)
        extra.append(b)
        extra_x.append(xb)
    tracks = np.ascontiguousarray(np.concatenate([tracks, np.stack(extra)]))
    X = np.concatenate([X, np.stack(extra_x)])
    return tracks, Ks, poses, X, planted_matches(tracks, Ks, poses), sizes


def equal_counts_scene(n=400, size=512, seed=7):
    """m = 4, spaced points: every track is seen in images 2 and 3, images 0 and 1 have identical visibility columns and
    the pair (0, 1) has no matches (a pair whose F was not found), so the two images are linked through the same rows:
    their counts tie and max_by_key must take image 1.  -> (tracks, K, poses, X, matches)."""
    rng = np.random.default_rng(seed + 1000)
    visible = np.ones((n, 4), dtype=bool)
    visible[:, 0] = visible[:, 1] = rng.random(n) < 0.6
    tracks, K, poses, X = multiview_scene(4, n, size, seed, visible=visible, spaced=True)
    matches = planted_matches(tracks, K, poses)
    del matches[(0, 1)]
    return tracks, K, poses, X, matches


def few_links_scene(n=400, size=512, seed=8):
    """m = 5, spaced points: image 3 is seen by two tracks only, and those by images 0 and 4 only, so image 3 ends with
    fewer than RANSAC_N linked tracks and its recover_pose fails at once.  No image can be placed AFTER such a failure (an
    image is taken when it has the most linked tracks, so whatever remains has at most two as well, and a failure places
    nothing that could add links): it is the last image tried.  -> (tracks, K, poses, X, matches)."""
    rng = np.random.default_rng(seed + 1000)
    visible = rng.random((n, 5)) >= 0.2
    visible[:, 3] = False
    visible[[5, 17]] = [True, False, False, True, True]
    tracks, K, poses, X = multiview_scene(5, n, size, seed, visible=visible, spaced=True)
    return tracks, K, poses, X, planted_matches(tracks, K, poses)


def scrambled_scene(n=150, size=512, seed=9):
    """m = 5, spaced points: image 3 is seen by every track but its points are random pixels, so it has the most linked
    tracks after the initial pair, is tried first, runs all 100 batches and fails; the others are placed after it.
    -> (tracks, K, poses, X, matches)."""
    rng = np.random.default_rng(seed + 1000)
    visible = rng.random((n, 5)) >= 0.25
    visible[:, 3] = True
    tracks, K, poses, X = multiview_scene(5, n, size, seed, bad_image=3, visible=visible, spaced=True)
    return tracks, K, poses, X, planted_matches(tracks, K, poses)


def restated_pairs(st, matches):
    """add_image_pair_sparse of a ref_pose.SparseTriangulation for every planted pair, in the driver's (sorted) order
    -> {(i, j): (p2, score)}."""
    return {ij: st.add_image_pair_sparse(ij[0], ij[1], F, rows) for ij, (rows, F) in sorted(matches.items())}


# ---- recover_pose runs past the first batch -----------------------------------------------------------------------------
# One scene, three thresholds: max_dimension is recover_pose's argument and the threshold is 5 % of it.  Measured with the
# restatement and the device's index stream (tests/test_pose_ref.py pins the first run, tests/golden/pose_runs.json
# records the others): 13 leaves after batch 3 of 100; 11 runs every batch and is accepted with a winner in batch 70;
# with image 2's points scrambled (at 512) every batch runs and the result is rejected.  The fourth run, stage_scrambled,
# is the failing call of scrambled_scene's sparse stage.
RANSAC_SCENE = {"m": 5, "n": 160, "seed": 9, "miss": 0.25, "image": 2, "placed": (0, 1, 4), "sample_seed": 5}
RANSAC_RUNS = {"middle_batch": {"scrambled": False, "max_dimension": 13},
               "accepted_late": {"scrambled": False, "max_dimension": 11},
               "scrambled_rejected": {"scrambled": True, "max_dimension": 512},
               "stage_scrambled": {"stage": "scrambled_scene", "stage_seed": 3, "max_dimension": 512}}


def ransac_scene(scrambled=False):
    """-> (tracks, K, P, has, image) of RANSAC_SCENE: the true projections of the placed images."""
    s = RANSAC_SCENE
    tracks, K, poses, _ = multiview_scene(s["m"], s["n"], seed=s["seed"], miss=s["miss"],
                                          bad_image=s["image"] if scrambled else None)
    P, has = known_views(K, poses, s["placed"])
    return tracks, K, P, has, s["image"]
