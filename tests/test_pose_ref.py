"""Pose recovery's restatement (tests/ref_pose.py) on the CPU: solve_quartic, P3P on exact triples, find_projection_matrix
on the planted geometry, the device generator's index stream."""
import numpy as np
import pytest

import ref_pose as rp
import ref_triangulation as rt
from cybervision_amd import synth


def test_solve_quartic_recovers_known_roots():
    rng = np.random.default_rng(1)
    for _ in range(200):
        roots = np.sort(rng.uniform(-3, 3, size=4))
        a = rng.uniform(0.5, 2.0)
        h = a * np.poly(roots)
        got = np.sort(np.asarray(rp.solve_quartic(h), dtype=np.float64))
        if not np.isfinite(got).all():
            continue  # the closed form's cube root of a negative number is NaN, as in the reference
        assert np.allclose(got, roots, atol=1e-5), (got, roots)


def test_p3p_recovers_true_pose_on_exact_triples():
    K, poses = synth.sfm_cameras(512)
    R, t = poses[2]
    rng = np.random.default_rng(2)
    k_inv = np.linalg.inv(K)
    hits = 0
    for _ in range(50):
        X = rng.uniform(-0.3, 0.3, size=(3, 3)) + np.array([0.0, 0.0, 1.0])
        q = (K @ (R @ X.T + t[:, None])).T
        samples = [(q[i, :2] / q[i, 2], X[i]) for i in range(3)]
        best = min((np.abs(Rc - R).max() + np.abs(tc - t).max() for _, Rc, tc in rp.recover_pose_from_points(k_inv, samples)),
                   default=np.inf)
        hits += best < 1e-9
    # the closed form takes powf(1/3) of negative numbers (NaN, as in the reference) on part of the triples, which then lose
    # the true root; measured 38 of these 50 recover it to 1e-9
    assert hits >= 35, hits


def test_find_projection_matrix_on_planted_geometry():
    K, poses = synth.sfm_cameras(512)
    F = synth.sfm_true_f(K, poses[0], poses[1])
    rng = np.random.default_rng(4)
    p0 = rng.uniform(40, 472, size=(500, 2))
    X = (np.linalg.inv(K) @ np.stack([p0[:, 0], p0[:, 1], np.ones(500)])).T * rng.uniform(0.8, 1.2, 500)[:, None]
    R, t = poses[1]
    q = (K @ (R @ X.T + t[:, None])).T
    tracks = np.stack([p0, q[:, :2] / q[:, 2:3]], axis=1)
    p2, count, counts = rp.find_projection_matrix(F, K, K, tracks)
    assert count == 500 and sorted(counts)[-2] < 500
    assert np.abs(p2[:, :3] - R).max() < 1e-9
    assert abs(abs(p2[:, 3] @ t) / np.linalg.norm(t) - 1.0) < 1e-9


def test_device_generator_stream():
    idx = [rp.device_samples(7, b, h, 1000) for b in range(3) for h in range(200)]
    flat = np.array(idx).ravel()
    assert flat.min() >= 0 and flat.max() < 1000 and len(np.unique(flat)) > 800
    assert idx == [rp.device_samples(7, b, h, 1000) for b in range(3) for h in range(200)]
    assert rp.device_samples(7, 0, 0, 1000) != rp.device_samples(8, 0, 0, 1000)


def test_restated_recover_pose_candidates_score_the_truth():
    import pose_scenes

    tracks, K, poses, X = pose_scenes.scene(n=300)
    P = [pose_scenes.projection(K, *poses[0]), pose_scenes.projection(K, *poses[1]), None]
    pts, ok, _ = rt.triangulate_tracks(tracks[:, :2], P[:2])
    lt, lp = rp.linked(tracks, pts, ok, 2)
    rng = np.random.default_rng(5)
    counts = [c[6] for _ in range(40) for c in rp.pose_candidates(lt, lp, P, 2, K, 512, list(rng.integers(0, len(lt), 3)))
              if c[5]]
    assert counts and max(counts) > 0.7 * len(lt)


def test_restated_recover_next_cameras_order_config5_512(oracle, oracle_fm):
    """Config 5's 512^2 sparse stage on the CPU (the oracle's ORB and matcher; the pairs' inliers are the matches that fit
    the planted F, since the reference's RANSAC is OS-seeded): the restated recover_next_cameras places the initial pair,
    then the third view, and recover_pose accepts it at the early-exit level."""
    from cybervision_amd import fundamentalmatrix

    size = 512
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    kps = []
    for pyr in pyrs:
        ost = int(oracle.lib().cvref_orb_optimal_scale_steps(size, size))
        xs, ds = [], []
        for i in range(ost + 1):
            k = ost - i
            xy, desc = oracle.orb_extract(pyr[k])
            xs.append(np.floor(xy.astype(np.float32) / np.float32(1.0 / (1 << k))).astype(np.uint32))
            ds.append(desc)
        kps.append((np.concatenate(xs), np.concatenate(ds)))
    st = rp.SparseTriangulation(3, [(size, size)] * 3, [K] * 3, oracle.extend_tracks)
    t = fundamentalmatrix.RANSAC_T_PERSPECTIVE * size
    for i, j in [(0, 1), (0, 2), (1, 2)]:
        m, _ = oracle.match_points(kps[i][0], kps[i][1], kps[j][0], kps[j][1], 48)
        F = synth.sfm_true_f(K, poses[i], poses[j])
        st.add_image_pair_sparse(i, j, F, m[oracle_fm.fits_model(F, m, t)])
    first = st.recover_next_cameras(seed=0)
    second = st.recover_next_cameras(seed=1)
    assert len(first) == 2 and len(second) == 1 and sorted(first + second) == [0, 1, 2]
    assert st.recover_next_cameras(seed=2) == []
    assert st.last is None


# ---- the scenes of tests/test_pose_multiview_gpu.py: each one shown, from the restatement alone, to exercise what it is for
def _near_threshold_margin(contenders, final_count):
    return min(mg for c, mg in contenders if c >= final_count - 1)


def test_multiview_scene_is_ragged_and_inside_the_image():
    import pose_scenes

    for m in range(2, 9):
        tracks, K, poses, X = pose_scenes.multiview_scene(m, 500, seed=30 + m, miss=0.3)
        again = pose_scenes.multiview_scene(m, 500, seed=30 + m, miss=0.3)[0]
        seen = tracks[..., 0] >= 0
        assert np.array_equal(tracks, again) and tracks[seen].min() >= 0 and tracks[seen].max() < 512
        assert (tracks[~seen] == -1).all() and 0.6 < seen.mean() < 0.8 and len(poses) == m
        for R, t in poses[1:]:
            assert 0.01 < np.linalg.norm(t) < 0.07 and np.arcsin(np.linalg.norm(R - R.T) / np.sqrt(8.0)) < 0.002
        # the planted matches fit the true F: x2^T F x1 = 0 up to the rounding to pixels
        for (i, j), (rows, F) in pose_scenes.planted_matches(tracks, K, poses).items():
            x1 = np.hstack([rows[:, :2], np.ones((len(rows), 1))])
            x2 = np.hstack([rows[:, 2:], np.ones((len(rows), 1))])
            line = x1 @ F.T
            dist = np.abs((x2 * line).sum(axis=1)) / np.linalg.norm(line[:, :2], axis=1)
            assert len(rows) == (seen[:, i] & seen[:, j]).sum() and dist.max() < 1.5, (m, i, j)


def test_per_sample_configs_cover_the_slots():
    """The configurations of the per-sample parity test: m in {3, 4, 6, 8}; the image first, in the middle and last; 2 to
    m - 1 known views; at m = 8 view 7 known alone with one other."""
    import pose_checks as pc

    assert {m for m, _, _ in pc.MULTIVIEW_CONFIGS} == {3, 4, 6, 8}
    assert (8, 7) in {(m, len(p)) for m, _, p in pc.MULTIVIEW_CONFIGS} and any(
        m == 8 and 7 in p and len(p) == 2 for m, _, p in pc.MULTIVIEW_CONFIGS)
    for m in (4, 6, 8):
        images = {i for mm, i, _ in pc.MULTIVIEW_CONFIGS if mm == m}
        assert 0 in images and m - 1 in images and images - {0, m - 1}
        assert {len(p) for mm, _, p in pc.MULTIVIEW_CONFIGS if mm == m} >= {2, m - 1}


def _per_sample_configs():
    import pose_checks as pc

    return pc.MULTIVIEW_CONFIGS


@pytest.mark.parametrize("m,image,placed", _per_sample_configs())
def test_per_sample_config_scores_enough_poses(m, image, placed):
    """A configuration of the per-sample parity test: more than 1000 poses pass the 3-sample check (every one of them is
    scored: the existing test's floor) and the linked tracks are seen in 2, in 3 and in more known views where that many
    are known."""
    import pose_checks as pc

    assert image not in placed
    tracks, K, P, has, projections = pc.multiview_config(m, image, placed)
    pts, ok = pc.restated_points(tracks, P, has)
    lt, lp = rp.linked(tracks, pts, ok, image)
    known = (lt[:, list(placed), 0] >= 0).sum(axis=1)
    assert (known == 2).any() and (len(placed) < 3 or (known == 3).any()) and (len(placed) < 4 or (known > 3).any())
    samples = pc.sample_triples(lp, pc.MULTIVIEW_TRIPLES)
    passed = sum(c[5] for s in samples for c in rp.pose_candidates(lt, lp, projections, image, K, 512, [int(v) for v in s],
                                                                   score=False))
    print(m, image, placed, len(lt), "linked,", passed, "poses pass the 3-sample check")
    assert passed > 1000 and len(lt) > 200, (m, image, placed, passed)


def test_middle_batch_scene_leaves_in_a_middle_batch():
    """pose_scenes' middle_batch run: accepted after 2..20 batches with a winner from a later batch than the first; the
    best after batch 0 is replaced, and a carried result survives at least one batch; no track of the winner or of a
    hypothesis within 1 of its count lies within 1e-6 * max_dimension of the threshold."""
    import pose_checks as pc

    tracks, pts, ok, projections, image, K, md, seed = pc.run_inputs("middle_batch")
    contenders = []

    def observe(_b, _h, _s, count, _e, errs):
        with np.errstate(all="ignore"):
            contenders.append((count, float(np.nanmin(np.abs(errs - rp.RANSAC_T * md)))))

    res = rp.recover_pose(tracks, pts, ok, projections, image, K, md, seed, observe=observe)
    winners = [w for _, _, w in res["history"]]
    print("middle batch:", res["count"], "of", res["linked"], "after", res["batches"], "batches, winners", winners)
    assert res["camera"] is not None and 2 <= res["batches"] <= 20 and res["winner"][0] >= 1
    assert winners[0] is not None and winners[0] != res["winner"]
    assert any(winners[k] == winners[k - 1] for k in range(1, len(winners)))
    assert res["count"] >= rp.RANSAC_D_PERCENT_EARLY_EXIT * res["linked"] // 100 > res["history"][-2][0]
    assert _near_threshold_margin(contenders, res["count"]) > 1e-6 * md


def test_pose_fixture_matches_restatement(oracle):
    """tests/golden/pose_runs.json against the restatement: the inputs' digest and linked count, batch 0 and the winner's
    batch re-derived from scratch; and what the recorded runs are for: 100 batches each, one accepted with a winner past
    batch 50 that replaced earlier ones, two rejected; no near-threshold track among the contenders."""
    import json
    from pathlib import Path

    import pose_checks as pc

    runs = json.loads((Path(__file__).resolve().parent / "golden" / "pose_runs.json").read_text())["runs"]
    assert set(runs) == {"accepted_late", "scrambled_rejected", "stage_scrambled"}
    for name, fx in runs.items():
        tracks, pts, ok, projections, image, K, md, seed = pc.run_inputs(name)
        lt, lp = rp.linked(tracks, pts, ok, image)
        assert pc.table_digest(tracks) == fx["table"] and len(lt) == fx["linked"] and (image, md, seed) == (
            fx["image"], fx["max_dimension"], fx["seed"])
        assert fx["ransac_d"] == rp.RANSAC_D_PERCENT * len(lt) // 100 and fx["batches"] == 100 == len(fx["history"])
        assert fx["accepted"] == (fx["count"] > fx["ransac_d"]) and fx["count"] < rp.RANSAC_D_PERCENT_EARLY_EXIT * len(lt) // 100
        assert fx["history"][-1] == [fx["count"], fx["error"], fx["winner"]] and fx["margin"] > 1e-6 * md
        for batch in sorted({0, fx["winner"][0]}):
            cam, count, error, winner = rp.recover_pose_batch(lt, lp, projections, image, K, md, seed, batch)
            if batch == 0:
                assert [count, list(winner)] == [fx["history"][0][0], fx["history"][0][2]]
                assert np.isclose(error, fx["history"][0][1], rtol=1e-9, atol=0)
            if batch == fx["winner"][0]:
                assert count == fx["count"] and list(winner) == fx["winner"] and np.isclose(error, fx["error"], rtol=1e-9, atol=0)
                for got, want in zip(cam, (fx["r"], fx["t"], fx["projection"])):
                    assert np.allclose(got, want, rtol=1e-9, atol=1e-12)
    late = runs["accepted_late"]
    changes = [k for k in range(100) if k == 0 or late["history"][k][2] != late["history"][k - 1][2]]
    assert late["accepted"] and late["winner"][0] >= 50 and len(changes) >= 3 and changes[-1] == late["winner"][0]
    assert not runs["scrambled_rejected"]["accepted"] and not runs["stage_scrambled"]["accepted"]
    assert runs["stage_scrambled"]["linked"] < 300  # (the failing image's table stays small: the generator's cost)


def _restated_stage(oracle, scene, recover=None, seed=3):
    import pose_scenes

    tracks, K, poses, _, matches = scene
    m = tracks.shape[1]
    st = rp.SparseTriangulation(m, [(512, 512)] * m, [K] * m, oracle.extend_tracks)
    pose_scenes.restated_pairs(st, matches)
    initial = st.best[1]
    order, calls = rp.recover_camera_poses(st, seed=seed, recover=recover)
    return st, initial, order, calls


def test_equal_counts_scene_ties_and_takes_the_later_image(oracle):
    import pose_scenes

    st, initial, order, calls = _restated_stage(oracle, pose_scenes.equal_counts_scene())
    assert initial == (2, 3) and order == [2, 3, 1, 0]
    assert calls[1]["counts"][0] == calls[1]["counts"][1] > 100 and calls[1]["image"] == 1
    assert all(c["pose"]["camera"] is not None for c in calls[1:])


def test_few_links_scene_fails_at_once_and_last(oracle):
    """Image 3 has fewer than RANSAC_N linked tracks: the restated recover_next_cameras raises for it without a batch.
    It is the last image tried (nothing can be placed after such a failure: see pose_scenes.few_links_scene), and the
    call still counts."""
    import pose_scenes

    st, initial, order, calls = _restated_stage(oracle, pose_scenes.few_links_scene())
    assert sorted(order) == [0, 1, 2, 4] and len(calls) == 4
    failed = calls[-1]
    assert "failure" in failed and failed["image"] == 3 and 0 < failed["pose"]["linked"] < rp.RANSAC_N
    assert failed["pose"]["batches"] == 0 and st.projections[3] is None
    assert all("failure" not in c for c in calls[:-1])


def test_scrambled_scene_fails_first_and_the_others_follow(oracle):
    """Image 3 (random points) has the most linked tracks after the initial pair, so it is tried first; its 100 batches
    are the fixture's stage_scrambled run (re-derived in part by test_pose_fixture_matches_restatement); the restated
    recover_next_cameras raises for it and the remaining images are placed after it."""
    import json
    from pathlib import Path

    import pose_checks as pc
    import pose_scenes

    fx = json.loads((Path(__file__).resolve().parent / "golden" / "pose_runs.json").read_text())["runs"]["stage_scrambled"]
    seeds = []

    def recover(tracks, points, ok, projections, image, K, md, seed):
        seeds.append((image, seed))
        if image != fx["image"]:
            return rp.recover_pose(tracks, points, ok, projections, image, K, md, seed)
        assert pc.table_digest(tracks) == fx["table"] and seed == fx["seed"] and md == fx["max_dimension"]
        return {"camera": None, "count": fx["count"], "batches": fx["batches"], "winner": tuple(fx["winner"]),
                "linked": fx["linked"]}

    st, initial, order, calls = _restated_stage(oracle, pose_scenes.scrambled_scene(), recover=recover)
    assert 3 not in initial and order == list(initial) + [c["image"] for c in calls[2:]] and len(order) == 4
    failed = calls[1]
    assert "failure" in failed and failed["image"] == 3 and failed["counts"][3] == fx["linked"] == max(failed["counts"].values())
    assert seeds == [(3, 4)] + [(c["image"], 3 + k) for k, c in enumerate(calls) if k >= 2]
    assert all(c["pose"]["camera"] is not None for c in calls[2:]) and st.projections[3] is None


def test_recover_camera_poses_keeps_the_failure_message_and_goes_on():
    """reconstruction.recover_camera_poses around a stand-in triangulation: a failed call is listed with its message under
    "failure" next to the call's own figures (whose "error" is recover_pose's residual, not the message), takes a seed
    like any other, and the loop goes on to the next image."""
    from cybervision_amd import _lib, reconstruction

    class Stub:
        def __init__(self):
            self.script = [[0, 1], None, [3], []]
            self.seeds, self.completed, self.last_pose = [], False, None

        def recover_next_cameras(self, device, seed=0):
            self.seeds.append(seed)
            step = self.script.pop(0)
            self.last_pose = None if step is None or len(step) != 1 else {"image": step[0], "error": 0.25, "count": 9}
            if step is None:
                self.last_pose = {"image": 2, "error": 0.5, "count": 4}
                raise _lib.CvhipError(-6, "cvhip_recover_pose", "Unable to find projection matrix")
            return step

        def complete_sparse_triangulation(self):
            self.completed = True

    tri, log = Stub(), []
    order, info = reconstruction.recover_camera_poses(None, tri, seed=7, log=log.append)
    assert order == [0, 1, 3] and tri.seeds == [7, 8, 9, 10] and tri.completed and len(log) == 1
    assert info[0] == {"images": [0, 1]} and info[2] == {"images": [3], "image": 3, "error": 0.25, "count": 9}
    assert "images" not in info[1] and "Unable to find projection matrix" in info[1]["failure"]
    assert info[1]["image"] == 2 and info[1]["error"] == 0.5 and info[1]["count"] == 4


# ---- the mixed scenes (a K and an image size per camera): tests/mixed_scenes.py ---------------------------------------------
def test_two_k_true_f_fits_the_mixed_projections():
    """mixed_scenes.true_f: x2^T F x1 = 0 for exact projections through K1 [R1 | t1] and K2 [R2 | t2] with K1 != K2; with
    the two K exchanged it does not hold; with one K it is synth.sfm_true_f."""
    import mixed_scenes
    import pose_scenes

    _, Ks, poses, X, _ = pose_scenes.mixed_multiview_scene(3, 200, seed=3, miss=0.0)
    for i in range(3):
        for j in range(3):
            if i == j:
                continue
            x1 = (pose_scenes.projection(Ks[i], *poses[i]) @ np.hstack([X, np.ones((len(X), 1))]).T).T
            x2 = (pose_scenes.projection(Ks[j], *poses[j]) @ np.hstack([X, np.ones((len(X), 1))]).T).T
            x1, x2 = x1 / x1[:, 2:], x2 / x2[:, 2:]

            def distance(F):
                line = x1 @ F.T
                return np.abs((x2 * line).sum(axis=1)) / np.linalg.norm(line[:, :2], axis=1)

            assert distance(mixed_scenes.true_f(Ks[i], Ks[j], poses[i], poses[j])).max() < 1e-8
            assert distance(mixed_scenes.true_f(Ks[j], Ks[i], poses[i], poses[j])).max() > 1.0
    K = Ks[0]
    assert np.allclose(mixed_scenes.true_f(K, K, poses[1], poses[2]), synth.sfm_true_f(K, poses[1], poses[2]), rtol=1e-12, atol=0)


def test_find_projection_matrix_tells_k1_from_k2():
    """The scene of test_find_projection_matrix_with_two_calibrations: on every ordered pair the restatement's winner
    beats the runner-up strictly (no tie for the SVD's signs to decide) and sees (nearly) every track in front of both
    cameras; called with the two K exchanged - E = K1^T F K2 - it finds another winner or a strictly lower score."""
    import mixed_scenes
    import pose_scenes

    tracks, Ks, poses, _, sizes = pose_scenes.mixed_multiview_scene(3, 3000, seed=3, miss=0.0)
    assert len(set(sizes)) == 3 and (tracks >= 0).all()
    for i, j in [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]:
        F = mixed_scenes.true_f(Ks[i], Ks[j], poses[i], poses[j])
        short = tracks[:, [i, j]]
        p2, count, counts = rp.find_projection_matrix(F, Ks[i], Ks[j], short)
        assert count > 0.99 * len(short) and sorted(counts)[-2] < count, (i, j, counts)
        R = poses[j][0] @ poses[i][0].T
        assert np.abs(p2[:, :3] - R).max() < 1e-9, (i, j)
        q2, qcount, qcounts = rp.find_projection_matrix(F, Ks[j], Ks[i], short)
        print((i, j), counts, "exchanged:", qcounts)
        assert qcount < count or np.abs(q2 - p2).max() > 1e-3, (i, j)


def _mixed_configs():
    import pose_checks as pc

    return pc.MIXED_CONFIGS


@pytest.mark.parametrize("m,image,placed", _mixed_configs())
def test_mixed_config_scores_enough_poses(m, image, placed):
    """A mixed configuration of the per-sample parity test, from the restatement alone: it is one of MULTIVIEW_CONFIGS,
    the image is not square, more than 1000 poses pass the 3-sample check (check_models' floor) over more than 200 linked
    tracks; and the image's own K matters - with camera 0's K in its place the first poses differ by far more than the
    comparison's 1e-6."""
    import pose_checks as pc

    assert (m, image, placed) in pc.MULTIVIEW_CONFIGS
    tracks, Ks, P, has, projections, sizes = pc.multiview_config_mixed(m, image, placed)
    size = max(sizes[image])
    assert size != min(sizes[image]) and len(set(sizes)) == m
    seen = tracks[..., 0] >= 0
    for j, (w, h) in enumerate(sizes):
        assert tracks[seen[:, j], j, 0].max() < w and tracks[seen[:, j], j, 1].max() < h
    pts, ok = pc.restated_points(tracks, P, has)
    lt, lp = rp.linked(tracks, pts, ok, image)
    samples = pc.sample_triples(lp, pc.MULTIVIEW_TRIPLES)
    passed = sum(c[5] for s in samples for c in rp.pose_candidates(lt, lp, projections, image, Ks[image], size,
                                                                   [int(v) for v in s], score=False))
    print("mixed", m, image, placed, len(lt), "linked,", passed, "poses pass the 3-sample check")
    assert passed > 1000 and len(lt) > 200
    differ = 0
    for s in samples[-20:]:  # (random triples: the special ones come first)
        own = rp.pose_candidates(lt, lp, projections, image, Ks[image], size, [int(v) for v in s], score=False)
        other = rp.pose_candidates(lt, lp, projections, image, Ks[0], size, [int(v) for v in s], score=False)
        differ += [c[0] for c in own] != [c[0] for c in other] or any(np.abs(a[4] - b[4]).max() > 1e-3 for a, b in zip(own, other))
    assert differ >= 15


def test_mixed_whole_call_leaves_after_the_first_batch():
    """pose_checks.mixed_run_inputs: the restated recover_pose is accepted after batch 0 with at least 95 % of more than
    300 linked tracks, no contender within 1 of the winner's count has a track within 1e-6 max_dimension of the
    threshold; with camera 0's K for the image's own it ends with another winner."""
    import pose_checks as pc

    tracks, K, P, has, image, pts, ok, md, seed, projections = pc.mixed_run_inputs()
    contenders = []

    def observe(_b, _h, _s, count, _e, errs):
        with np.errstate(all="ignore"):
            contenders.append((count, float(np.nanmin(np.abs(errs - rp.RANSAC_T * md)))))

    res = rp.recover_pose(tracks, pts, ok, projections, image, K, md, seed, observe=observe)
    print("mixed whole call:", res["count"], "of", res["linked"], "after", res["batches"], "batch(es), winner", res["winner"])
    assert res["camera"] is not None and res["batches"] == 1 and res["linked"] > 300
    assert res["count"] >= rp.RANSAC_D_PERCENT_EARLY_EXIT * res["linked"] / 100
    assert _near_threshold_margin(contenders, res["count"]) > 1e-6 * md
    k0 = pc.multiview_config_mixed(*pc.MIXED_RUN["config"])[1][0]
    other = rp.recover_pose(tracks, pts, ok, projections, image, k0, md, seed)
    assert other["winner"] != res["winner"] or other["count"] != res["count"]


def test_sparse_mixed_scene_tells_the_images_apart(oracle):
    """pose_scenes.sparse_mixed_scene through the restated stage: no two image sizes alike, landscape and portrait, only
    image 2 has a side past 1000 pixels (extend_tracks' radius is 4 for pairs ending in image 2, else 3); every pixel
    lies inside its image and inside the images before it; every pair's find_projection_matrix has a strict winner; all
    four cameras are placed, each recover_pose in one batch.  The table hangs on whose size gives the radius: with image
    1's longer side in place of image 2's, extend_tracks builds another table."""
    import pose_scenes

    tracks, Ks, poses, _, matches, sizes = pose_scenes.sparse_mixed_scene()
    assert len(set(sizes)) == 4 and any(w > h for w, h in sizes) and any(w < h for w, h in sizes)
    assert [3 * max(s) // 1000 if max(s) > 1000 else 3 for s in sizes] == [3, 3, 4, 3]
    seen = tracks[..., 0] >= 0
    for j in range(4):
        for i in range(j + 1):
            assert tracks[seen[:, j], j, 0].max() < sizes[i][0] and tracks[seen[:, j], j, 1].max() < sizes[i][1], (i, j)
    assert len(matches) == 6

    def stage(extend):
        st = rp.SparseTriangulation(4, sizes, Ks, extend)
        pairs = pose_scenes.restated_pairs(st, matches)
        return st, pairs, st.tracks.copy()

    st, pairs, table = stage(oracle.extend_tracks)
    for (i, j), (rows, F) in matches.items():
        both = (table[:, i, 0] >= 0) & (table[:, j, 0] >= 0)
        counts = rp.find_projection_matrix(F, Ks[i], Ks[j], table[both][:, [i, j]])[2]
        assert sorted(counts)[-2] < max(counts) == pairs[(i, j)][1], (i, j, counts)
    order, calls = rp.recover_camera_poses(st, seed=3)
    print("mixed_4:", len(table), "tracks, order", order, [(c["image"], c["pose"] and (c["pose"]["linked"], c["pose"]["count"],
                                                                                       c["pose"]["batches"])) for c in calls])
    assert sorted(order) == [0, 1, 2, 3] and all("failure" not in c for c in calls)
    assert all(c["pose"]["batches"] == 1 for c in calls[1:])
    # the planted companions: their match is taken into the neighbour's track in the pair (0, 2) only
    n = len(tracks) - 12
    for k in range(12):
        a, b = tracks[k], tracks[n + k]
        other = 2 if k % 2 == 0 else 3
        merged = ((table[:, 0] == a[0]).all(axis=1) & (table[:, other] == b[other]).all(axis=1)).any()
        alone = ((table[:, 0] == b[0]).all(axis=1) & (table[:, other] == b[other]).all(axis=1)).any()
        assert merged == (other == 2) and alone, k  # (B keeps a track of its own: the merged match is cleared at its image-2 pixel)
    # image 1's longer side for image 2's: radius 3 for (0, 2) and (1, 2), 4 for (2, 3)
    _, _, wrong = stage(lambda grid, tp1, max_dimension: oracle.extend_tracks(grid, tp1, max(grid.shape[:2])))
    assert wrong.shape != table.shape or not np.array_equal(wrong, table)
