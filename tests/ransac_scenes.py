"""Match lists for the sampler restatement and the RANSAC replay tests (generated, deterministic)."""
import math

import numpy as np

BAND_X1 = 500  # the cluster scenes' band: x1 in [500, 508] - any two of its matches are closer than 10 px in x1


def _far_points(k, rng):
    """k matches more than 10 px from each other in every coordinate and more than 10 px in x1 from the band, on the
    exact affine geometry y2 = y1 + 7 with varying disparities (so that four of them span a model)."""
    x1 = 40 + 100 * np.arange(k)                      # 40, 140, ..: none within 30 of the band
    y1 = 30 + 90 * rng.permutation(k)
    x2 = x1 + rng.integers(-40, 41, size=k)           # spacing stays >= 20
    return np.stack([x1, y1, x2, y1 + 7], axis=1)


def cluster_matches(n, k, seed=3, blocker=False):
    """All but k matches inside a 9-pixel band of x1, k matches far from each other in every coordinate, all on the
    exact geometry y2 = y1 + 7 (integer coordinates).  A sample holds at most ONE match of the band, so it needs
    n - 1 of the k far ones: most draws are rejected and part of the samples are given up.  The far matches are
    spread through the list.  blocker: the first far match sits at x1 = BAND_X1 + 9, within 10 px of the whole band -
    a sample can then hold k - 1 far matches and one of the band, or the k far ones, never more."""
    rng = np.random.default_rng(seed)
    far = _far_points(k, rng)
    if blocker:
        far[0, 0] = BAND_X1 + 9
        far[0, 2] = far[0, 0] + 15
        assert (np.abs(far[1:, [0]] - far[0, 0]) >= 10).all() and (np.abs(far[1:, [2]] - far[0, 2]) >= 10).all()
    nb = n - k
    bx1 = BAND_X1 + rng.integers(0, 9, size=nb)
    by1 = rng.integers(20, 1900, size=nb)
    bx2 = bx1 + rng.integers(-60, 61, size=nb)
    band = np.stack([bx1, by1, bx2, by1 + 7], axis=1)
    m = np.empty((n, 4), dtype=np.int64)
    at = np.linspace(0, n - 1, k).astype(np.int64)   # the far ones' places in the list
    is_far = np.zeros(n, dtype=bool)
    is_far[at] = True
    m[is_far] = far
    m[~is_far] = band
    d = np.abs(far[:, None, :] - far[None, :, :]) + 1000 * np.eye(k, dtype=np.int64)[:, :, None]
    assert (d >= 10).all()
    return m.astype(np.uint32), is_far


def exact_affine_matches(n, inlier_frac=1.0, seed=4):
    """A rectified pair in integer coordinates: y2 = y1 + 7 exactly for the inliers (x2 = x1 + a random disparity),
    uniform outliers for the rest.  Every sample of four inliers gives a model that accepts exactly the inliers:
    thousands of hypotheses tie at the maximal count in every round."""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(50, 1950, size=n)
    y1 = rng.integers(50, 1950, size=n)
    x2 = x1 + rng.integers(-80, 81, size=n)
    y2 = y1 + 7
    out = rng.random(n) >= inlier_frac
    x2[out] = rng.integers(0, 2000, size=int(out.sum()))
    y2[out] = rng.integers(0, 2000, size=int(out.sum()))
    return np.stack([x1, y1, x2, y2], axis=1).astype(np.uint32), ~out


def spread_exact_affine(n=14, seed=6):
    """n exact matches (y2 = y1 + 7) mutually more than 10 px apart in every coordinate."""
    rng = np.random.default_rng(seed)
    x1 = 60 + 45 * rng.permutation(n)
    y1 = 80 + 37 * rng.permutation(n)
    x2 = 30 + 52 * rng.permutation(n)
    return np.stack([x1, y1, x2, y1 + 7], axis=1).astype(np.uint32)


def tilt_matches(n, outlier_frac=0.35, seed=5, inliers_last=False):
    """The 12-degree tilted affine geometry of test_orb_ransac_gpu.affine_matches (rounded to integer pixels).
    inliers_last: the outliers are moved to the front of the list - with n > 5000 the matches past the first 5000 are
    then nearly all inliers, so a sampler that read past 5000 would draw different (and better) samples."""
    rng = np.random.default_rng(seed)
    th = math.radians(12.0)
    x1 = rng.integers(100, 1900, size=n).astype(np.float64)
    y1 = rng.integers(100, 1900, size=n).astype(np.float64)
    dist = rng.uniform(-80, 80, size=n)
    x2 = x1 + dist * math.cos(th)
    y2 = y1 + dist * math.sin(th)
    out = rng.random(n) < outlier_frac
    x2[out] = rng.integers(0, 2000, size=int(out.sum()))
    y2[out] = rng.integers(0, 2000, size=int(out.sum()))
    m = np.stack([x1, y1, np.round(x2), np.round(y2)], axis=1).clip(0, None).astype(np.uint32)
    if inliers_last:
        order = np.argsort(~out, kind="stable")  # outliers (True -> False) first
        m, out = m[order], out[order]
    return m, ~out


def exit_scene(noise=2, n=50_400, outliers=150, seed=41):
    """Perspective matches for the early exit above 50 000 inliers: n matches, `outliers` of them wrong - all inside
    the first 5000, the part of the list the sampler draws from.  That head also holds the inliers nearest the image
    centre, with their second point moved by up to `noise` pixels (still inliers of the true geometry at
    t = 0.01 * 2048): samples of them constrain the geometry poorly, so a hypothesis that accepts more than 50 000
    matches takes a few rounds to turn up."""
    import cases

    m = cases.perspective_matches(n=n, outlier_frac=0.0, seed=seed)[0].astype(np.int64)
    rng = np.random.default_rng(seed + 1)
    m = m[np.argsort(np.abs(m[:, :2] - 1024).max(axis=1), kind="stable")]
    m[:5000, 2:] += rng.integers(-noise, noise + 1, size=(5000, 2))
    bad = rng.choice(5000, size=outliers, replace=False)
    m[bad, 2:] = rng.integers(0, 2048, size=(outliers, 2))
    m[:5000] = m[:5000][rng.permutation(5000)]
    return np.ascontiguousarray(m.clip(0, 2047).astype(np.uint32))
