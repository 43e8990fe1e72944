"""Synthetic scenes for the pose-recovery tests: config 5's cameras (synth.sfm_cameras) looking at random points, and
rigs of 2 to 8 cameras with ragged tracks, planted matches per pair and the special scenes of the multi-view tests (what
each one is for is shown on the CPU by tests/test_pose_ref.py)."""
import numpy as np

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


def planted_matches(tracks, K, poses):
    """-> {(i, j): (matches [k, 4] uint32 (x1, y1, x2, y2), F)} for every pair i < j: the tracks seen in both images, in
    table order, and the true fundamental matrix (synth.sfm_true_f).  A pair without a common track is left out, as the
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
            out[(i, j)] = (np.ascontiguousarray(rows), synth.sfm_true_f(K, poses[i], poses[j]))
    return out


def known_views(K, poses, placed):
    """-> (P [m, 3, 4] with zeros where unknown, has [m] uint8) for the images in `placed`."""
    m = len(poses)
    P = np.zeros((m, 3, 4))
    has = np.zeros(m, dtype=np.uint8)
    for j in placed:
        P[j] = projection(K, *poses[j])
        has[j] = 1
    return np.ascontiguousarray(P), has


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
