"""The host restatement of the RANSAC loops' sampler (tests/ref_ransac_sampler.py) on its own: the rules the device
loops are then replayed with (tests/test_ransac_replay_gpu.py).  No GPU."""
import numpy as np
import pytest

import ransac_scenes
import ref_pose
import ref_ransac_sampler as rs


def test_mix64_is_the_pose_sampler_s():
    vals = [0, 1, 7, 0x9E3779B97F4A7C15, 2 ** 64 - 1, (5 << 32) | 49_999, 0x0123456789ABCDEF]
    for v in vals:
        assert int(rs.mix64(v)) == ref_pose.mix64(v)
    arr = rs.mix64(np.array(vals, dtype=np.uint64))
    assert [int(a) for a in arr] == [ref_pose.mix64(v) for v in vals]
    assert int(rs.GOLDEN) == 0x9E3779B97F4A7C15


def _honours_rule(m, idx):
    pts = m.astype(np.int64)[idx]                                   # [B, n, 4]
    d = np.abs(pts[:, :, None, :] - pts[:, None, :, :])
    n = idx.shape[1]
    d[:, np.arange(n), np.arange(n), :] = 1 << 20
    return (d >= rs.MIN_PIXEL_DISTANCE).all(axis=(1, 2, 3))


@pytest.mark.parametrize("n_matches", [14, 300, 5000, 5200])
@pytest.mark.parametrize("n,tries", [(4, rs.TRIES_AFFINE), (7, rs.TRIES_PERSPECTIVE)])
def test_indices_stay_below_the_limit_and_samples_honour_the_rule(n_matches, n, tries):
    m, _ = ransac_scenes.tilt_matches(n_matches, seed=n_matches)
    limit = rs.limit_of(n_matches)
    assert limit == min(n_matches, 5000)
    idx, filled = rs.draw(m, limit, seed=7, round=2, H=4000, n=n, max_tries=tries)
    assert idx.shape == (4000, n) and idx.dtype == np.uint32
    assert (idx < limit).all()                  # for N = 5200: none is 5000 or more
    if n_matches >= 300:
        assert filled.mean() > 0.99 and idx.max() >= limit - 1 - limit // 50  # ... and the whole head is drawn from
    assert filled.any()
    assert _honours_rule(m, idx[filled]).all()  # all four coordinates, every pair of the sample
    for col in range(4):                        # each coordinate alone is enforced: no filled sample is close in it
        pts = m.astype(np.int64)[idx[filled]][:, :, col]
        d = np.abs(pts[:, :, None] - pts[:, None, :]) + (1 << 20) * np.eye(n, dtype=np.int64)
        assert d.min() >= 10


def test_draws_depend_on_seed_round_and_sample_index_only():
    m, _ = ransac_scenes.tilt_matches(3000)
    a, fa = rs.draw(m, 3000, seed=7, round=3, H=512, n=7, max_tries=512)
    b, fb = rs.draw(m, 3000, seed=7, round=3, H=200, n=7, max_tries=512)
    assert (a[:200] == b).all() and (fa[:200] == fb).all()      # sample h does not depend on the launch's size
    c, _ = rs.draw(m, 3000, seed=7, round=4, H=512, n=7, max_tries=512)
    d, _ = rs.draw(m, 3000, seed=8, round=3, H=512, n=7, max_tries=512)
    assert (a != c).any(axis=1).mean() > 0.99 and (a != d).any(axis=1).mean() > 0.99
    # the first draw of sample h, by hand
    h = 5
    state = ref_pose.mix64(7 ^ ref_pose.mix64((3 << 32) | h))
    state = ref_pose.mix64((state + 0x9E3779B97F4A7C15) & ref_pose.M64)
    assert a[h, 0] == ((state >> 32) * 3000) >> 32


def test_a_rejected_draw_is_skipped_not_retried_in_place():
    """Two matches only 5 px apart in y2 and nothing else close: no sample holds both."""
    m = ransac_scenes.spread_exact_affine(14).copy()
    m[3, 3] = m[9, 3] + 5
    idx, filled = rs.draw(m, 14, seed=1, round=0, H=3000, n=4, max_tries=256)
    assert filled.all()
    both = (idx == 3).any(axis=1) & (idx == 9).any(axis=1)
    assert not both.any() and (idx == 3).any() and (idx == 9).any()


# (N, k, n, tries): shares measured with the issue's scenes were 0.57, 0.61 and 0.50
CLUSTERS = [(300, 7, 7, rs.TRIES_PERSPECTIVE), (300, 5, 4, rs.TRIES_AFFINE), (1200, 14, 4, rs.TRIES_AFFINE)]


@pytest.mark.parametrize("n_matches,k,n,tries", CLUSTERS)
def test_cluster_scenes_leave_samples_unfilled(n_matches, k, n, tries):
    m, is_far = ransac_scenes.cluster_matches(n_matches, k)
    assert is_far.sum() == k and np.ptp(m[~is_far, 0].astype(np.int64)) <= 8
    idx, filled = rs.draw(m, rs.limit_of(n_matches), seed=7, round=0, H=10_000, n=n, max_tries=tries)
    share = filled.mean()
    print(f"N = {n_matches}, k = {k}, n = {n}, {tries} tries: {share:.3f} of the samples filled")
    assert 0.05 <= share <= 0.95
    assert _honours_rule(m, idx[filled]).all()
    assert (~is_far[idx[filled]]).sum(axis=1).max() <= 1   # at most one match of the band per sample


def test_degenerate_cluster_fills_no_sample():
    m, is_far = ransac_scenes.cluster_matches(1200, 3, blocker=True)
    idx, filled = rs.draw(m, 1200, seed=7, round=0, H=2000, n=4, max_tries=rs.TRIES_AFFINE)
    assert not filled.any()
