"""Synthetic scenes for the pose-recovery tests: config 5's cameras (synth.sfm_cameras) looking at random points."""
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
