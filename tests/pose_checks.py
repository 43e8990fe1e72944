"""What the pose tests share: the sample triples of the per-sample parity, its configurations at every view count, the
comparison of cvhip_recover_pose_models with ref_pose.pose_candidates (the rules and bounds of
test_pose_models_match_restatement_per_sample, which calls it too), and the inputs of the recover_pose runs that the
tests, the fixture generator (tests/tools/gen_pose_golden.py) and the fixture's CPU check all start from."""
import ctypes as C
import hashlib

import numpy as np

import pose_scenes
import ref_pose as rp
import ref_triangulation as rt

# (m, image_index, known views): image first, middle and last; 2 to m - 1 known views; at m = 8 bit 7 with one other
MULTIVIEW_CONFIGS = [
    (3, 0, (1, 2)), (3, 1, (0, 2)),
    (4, 1, (0, 2, 3)), (4, 3, (0, 1)), (4, 0, (2, 3)),
    (6, 3, (0, 1, 5)), (6, 0, (1, 2, 3, 4, 5)), (6, 5, (1, 3)),
    (8, 0, (1, 2, 3, 4, 5, 6, 7)), (8, 7, (0, 4)), (8, 4, (3, 7)), (8, 2, (0, 1, 5, 6)),
]
MULTIVIEW_TRACKS = 700
MULTIVIEW_TRIPLES = 2000


def _p(a):
    return C.c_void_p(a.ctypes.data)


def multiview_config(m, image, placed, size=512):
    """-> (tracks, K, P, has, projections as the restatement takes them) of a per-sample configuration: ragged tracks
    (miss 0.3) of rig(m), the true projections of `placed`."""
    tracks, K, poses, _ = pose_scenes.multiview_scene(m, MULTIVIEW_TRACKS, size, seed=20 + m, miss=0.3)
    P, has = pose_scenes.known_views(K, poses, placed)
    return tracks, K, P, has, [P[j] if has[j] else None for j in range(m)]


# one configuration of MULTIVIEW_CONFIGS per view count whose image is not square (mixed_scenes.dims(m, 4)): image 1 is
# 320 x 512, image 3 256 x 384, image 7 320 x 256
MIXED_CONFIGS = [(3, 1, (0, 2)), (6, 3, (0, 1, 5)), (8, 7, (0, 4))]


def multiview_config_mixed(m, image, placed):
    """multiview_config with a K and a size per image (pose_scenes.mixed_multiview_scene, the same seed, tracks and miss)
    -> (tracks, Ks [m], P, has, projections as the restatement takes them, sizes [m] (width, height)): the projections
    of `placed` use their own K; the recovered image's K is Ks[image] and its max_dimension max(sizes[image])."""
    tracks, Ks, poses, _, sizes = pose_scenes.mixed_multiview_scene(m, MULTIVIEW_TRACKS, seed=20 + m, miss=0.3)
    P, has = pose_scenes.known_views(Ks, poses, placed)
    return tracks, Ks, P, has, [P[j] if has[j] else None for j in range(m)], sizes


MIXED_RUN = {"config": (6, 3, (0, 1, 5)), "sample_seed": 5}


def mixed_run_inputs():
    """The inputs of the whole cvhip_recover_pose call on mixed cameras: MIXED_RUN's configuration, points from the
    restatement -> (tracks, K of the image, P, has, image, points, ok, max_dimension, seed, projections (None = unknown))."""
    m, image, placed = MIXED_RUN["config"]
    tracks, Ks, P, has, projections, sizes = multiview_config_mixed(m, image, placed)
    pts, ok = restated_points(tracks, P, has)
    return tracks, Ks[image], P, has, image, pts, ok, max(sizes[image]), MIXED_RUN["sample_seed"], projections


def restated_points(tracks, P, has):
    masked = np.array(tracks)
    masked[:, np.asarray(has) == 0] = -1
    pts, ok, _ = rt.triangulate_tracks(masked, list(P))
    return pts, ok


def table_digest(tracks):
    return hashlib.sha256(np.ascontiguousarray(tracks, dtype=np.int32).tobytes()).hexdigest()[:16]


def run_inputs(name):
    """The inputs of a recover_pose run of pose_scenes.RANSAC_RUNS, points from the restatement
    -> (tracks, points, ok, projections (None = unknown), image, K, max_dimension, seed).  stage_scrambled: the state of
    the restated sparse stage on scrambled_scene after the initial pair, its second call's image and seed."""
    run = pose_scenes.RANSAC_RUNS[name]
    if "stage" in run:
        from oracle import cvref

        cvref.build()
        tracks, K, poses, _, matches = getattr(pose_scenes, run["stage"])()
        m = tracks.shape[1]
        st = rp.SparseTriangulation(m, [(512, 512)] * m, [K] * m, cvref.extend_tracks)
        pose_scenes.restated_pairs(st, matches)
        st.recover_next_cameras(seed=run["stage_seed"])
        seen = {}

        def stop(*args):
            seen["args"] = args
            return {"camera": None}

        try:
            st.recover_next_cameras(seed=run["stage_seed"] + 1, recover=stop)
        except rt.TriangulationError:
            pass
        return seen["args"]
    tracks, K, P, has, image = pose_scenes.ransac_scene(run["scrambled"])
    pts, ok = restated_points(tracks, P, has)
    return (tracks, pts, ok, [P[j] if has[j] else None for j in range(len(has))], image, K, run["max_dimension"],
            pose_scenes.RANSAC_SCENE["sample_seed"])


def sample_triples(lp, B, seed=9, noise_triples=False):
    """B index triples into the linked tracks: random, the first B / 30 with the first index repeated in the second
    place, the next B / 60 with it repeated in the third, the next B / 12 near-collinear (the third point the closest to
    the middle of the first two).
    Those two kinds of duplicate give NaN on every path (a = 0, or a zero cross product).  The third kind, (i, j, j) with
    i != j, does not: x10 == x20 exactly, so c = ny . x20 is the rounding residue of a cross product of parallel vectors,
    q - 1 and p - 1 are residues too, and the quartic's coefficients are products of them (h = [-2.2e-16, 4.4e-16, 0, 0, 0]
    on one such triple).  Which of its roots are finite is decided by the last bit of each operation, fused
    multiply-adds included, so neither the reference nor any restatement defines an answer to compare with (DESIGN.md
    4.9).  Unless noise_triples is set, a random triple of that kind gets its third index from its first instead, which
    turns it into the second kind."""
    rng = np.random.default_rng(seed)
    samples = rng.integers(0, len(lp), size=(B, 3)).astype(np.uint32)
    if not noise_triples:
        noise = (samples[:, 1] == samples[:, 2]) & (samples[:, 0] != samples[:, 1])
        samples[noise, 2] = samples[noise, 0]
    d1, d2, c = B // 30, B // 30 + B // 60, B // 30 + B // 60 + B // 12
    samples[:d1, 1] = samples[:d1, 0]
    samples[d1:d2, 2] = samples[d1:d2, 0]
    for b in range(d2, c):
        i0, i1 = samples[b, 0], samples[b, 1]
        dist = np.linalg.norm(lp - 0.5 * (lp[i0] + lp[i1]), axis=1)
        dist[[i0, i1]] = np.inf
        samples[b, 2] = np.argmin(dist)
    return np.ascontiguousarray(samples)


def device_models(dev, tracks, pts, ok, P, has, image, K, size, samples):
    from cybervision_amd import _lib

    B = len(samples)
    n, m = tracks.shape[:2]
    pose, status = np.zeros((B, 4, 27)), np.zeros((B, 4), dtype=np.int8)
    count, err = np.zeros((B, 4), dtype=np.uint32), np.zeros((B, 4))
    tr, pt = np.ascontiguousarray(tracks), np.ascontiguousarray(pts)
    okb = np.ascontiguousarray(np.asarray(ok).astype(np.uint8))
    Pc, hc, Kc = np.ascontiguousarray(P), np.ascontiguousarray(has, dtype=np.uint8), np.ascontiguousarray(K)
    _lib.check(_lib.lib().cvhip_recover_pose_models(dev.handle, _p(tr), n, m, _p(pt), _p(okb), _p(Pc), _p(hc), image, _p(Kc),
                                                    size, _p(samples), B, _p(pose), _p(status), _p(count), _p(err)),
               "models")
    return pose, status, count, err


def check_models(got, lt, lp, projections, image, K, size, samples, label=""):
    """cvhip_recover_pose_models' outputs `got` against ref_pose.pose_candidates on every triple: the same root slots in
    order, R, t, the Camera's r and projection to 1e-9 (1e-6 for at most 1 % of the poses, those of ill-conditioned
    triples), the same 3-sample verdicts; counts exact and the largest residual to 1e-9 of the image size once the tracks
    whose error lies within that distance of the threshold are set aside: the count may differ by at most their number,
    and the error is compared where there is none.  -> (poses seen, loose, scored, exact)."""
    pose, status, count, err = got
    B = len(samples)
    thr = rp.RANSAC_T * size
    scored = exact = loose = poses_seen = 0
    loose_at = []
    for b in range(B):
        want = rp.pose_candidates(lt, lp, projections, image, K, size, [int(v) for v in samples[b]], per_track=True)
        assert [k for k in range(4) if status[b, k] != 0] == [w[0] for w in want], (label, b)
        # ill-conditioned triples (the near-collinear ones, and some random ones) amplify the last-bit differences of the
        # device's pow / sqrt / atan2 through the closed form's cancellations: every pose must match to 1e-6, at least 99 %
        # of them to 1e-9, and a pose's score is compared at the tolerance its pose met
        for slot, R, t, r, Pw, passed, cnt, e, errs in want:
            g = pose[b, slot]
            want_vec = np.concatenate([R.ravel(), t, r, Pw.ravel()])
            tight = np.allclose(g, want_vec, rtol=1e-9, atol=1e-9)
            rtol = 1e-9 if tight else 1e-6
            if not tight:
                loose += 1
                loose_at.append((b, slot, [int(v) for v in samples[b]]))
            poses_seen += 1
            assert np.allclose(g[:9], R.ravel(), rtol=1e-6, atol=1e-12), (label, b)
            assert np.allclose(g[9:12], t, rtol=1e-6, atol=1e-12), (label, b)
            assert np.allclose(g[12:15], r, rtol=1e-6, atol=1e-12), (label, b)
            assert np.allclose(g[15:], Pw.ravel(), rtol=1e-6, atol=1e-9), (label, b)
            assert (status[b, slot] == 2) == passed, (label, b)
            if not passed:
                continue
            scored += 1
            near = int((np.abs(errs - thr) <= rtol * size).sum())
            assert abs(int(count[b, slot]) - cnt) <= near, (label, b)
            if near == 0:
                exact += 1
                assert count[b, slot] == cnt, (label, b)
                # the error is a reprojection residual, a difference of pixel coordinates up to the image size: compared
                # in pixels (the largest residual, error * count) at rtol times the image size
                assert abs(err[b, slot] * cnt - e * cnt) <= rtol * size or (np.isnan(err[b, slot]) and np.isnan(e)), (label, b)
    print(f"{label}{B} triples, {poses_seen} poses ({loose} matched to 1e-6 only: {loose_at[:8]}), {scored} scored, "
          f"{exact} without a near-threshold track")
    assert scored > 1000 and exact > 0.9 * scored and loose <= 0.01 * poses_seen, (label, scored, exact, loose, loose_at)
    return poses_seen, loose, scored, exact


def device_recover_pose(dev, tracks, pts, ok, P, has, image, K, max_dimension, seed):
    """cvhip_recover_pose -> (rc, dict(count, error, batches, winner, r, t, projection))."""
    from cybervision_amd import _lib

    n, m = tracks.shape[:2]
    r, t, pr = np.zeros(3), np.zeros(3), np.zeros((3, 4))
    cnt, err, bat = C.c_uint32(0), C.c_double(0), C.c_uint32(0)
    winner = np.full(3, -7, dtype=np.int32)
    tr, pt = np.ascontiguousarray(tracks), np.ascontiguousarray(pts)
    okb = np.ascontiguousarray(np.asarray(ok).astype(np.uint8))
    Pc, hc, Kc = np.ascontiguousarray(P), np.ascontiguousarray(has, dtype=np.uint8), np.ascontiguousarray(K)
    rc = _lib.lib().cvhip_recover_pose(dev.handle, _p(tr), n, m, _p(pt), _p(okb), _p(Pc), _p(hc), image, _p(Kc),
                                       max_dimension, seed, _p(r), _p(t), _p(pr), C.byref(cnt), C.byref(err), C.byref(bat),
                                       _p(winner), _lib.NULL_PROGRESS, None)
    return rc, {"count": int(cnt.value), "error": float(err.value), "batches": int(bat.value),
                "winner": tuple(int(v) for v in winner), "r": r, "t": t, "projection": pr}
