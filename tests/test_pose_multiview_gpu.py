"""Pose recovery on the device past three views and past the first RANSAC batch: every view count, image slot and set of
known views against the restatement (tests/ref_pose.py, tests/ref_triangulation.py); runs that leave in a middle batch
or take all 100 (tests/golden/pose_runs.json); the sparse stage from planted matches with 4, 5 and 8 images.  The scenes
and what each is for: tests/pose_scenes.py, pinned on the CPU by tests/test_pose_ref.py."""
import json
from pathlib import Path

import numpy as np
import pytest

import pose_checks as pc
import pose_scenes
import ref_pose as rp
import ref_triangulation as rt
from cybervision_amd import _lib, reconstruction, triangulation

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "pose_runs.json"
_p = pc._p


def _has_patterns(m):
    """No view, each single view, two, some and all views known; at m = 8 bit 7 alone with one other."""
    pats = [[0] * m, [1] * m]
    pats += [[int(j == k) for j in range(m)] for k in (0, m - 1)]
    pats += [[int(j in (0, m - 1)) for j in range(m)], [int(j in (m // 2, m - 1)) for j in range(m)]]
    if m > 3:
        pats += [[j % 2 for j in range(m)], [int(j != 1) for j in range(m)]]
    if m == 8:
        pats += [[int(j in (3, 7)) for j in range(m)], [int(j >= 4) for j in range(m)]]
    return [np.array(h, dtype=np.uint8) for h in pats]


def _triangulate(dev, tracks, m, P, has, fill=-5.0):
    n = len(tracks)
    pts, ok = np.full((max(n, 1), 3), fill), np.full(max(n, 1), 9, dtype=np.uint8)
    tr = np.ascontiguousarray(tracks)
    rc = _lib.lib().cvhip_triangulate_tracks(dev.handle, _p(tr) if n else None, n, m, _p(P), _p(has), _p(pts), _p(ok))
    return rc, pts, ok


def test_triangulate_tracks_every_view_count(gpu_device):
    """cvhip_triangulate_tracks at m = 2..8, with no, one, two, some and all views known, ragged tracks, and table sizes
    around one block of 256: ok equal to ref_triangulation.triangulate_tracks on the masked table, points to 1e-9."""
    for m in range(2, 9):
        full, K, poses, _ = pose_scenes.multiview_scene(m, 3000, seed=30 + m, miss=0.3)
        allP = np.stack([pose_scenes.projection(K, R, t) for R, t in poses])
        for n in (0, 1, 255, 256, 257, 3000):
            tracks = full[:n]
            for has in _has_patterns(m):
                P = np.ascontiguousarray(allP * has[:, None, None])
                rc, pts, ok = _triangulate(gpu_device, tracks, m, P, has)
                assert rc == 0, (m, n, has)
                masked = tracks.copy()
                masked[:, has == 0] = -1
                wpts, wok, _ = rt.triangulate_tracks(masked, list(P))
                ok = ok[:n].astype(bool)
                assert np.array_equal(ok, wok), (m, n, has)
                assert has.sum() >= 2 or not ok.any()
                assert np.allclose(pts[:n][ok], wpts[ok], rtol=1e-9, atol=1e-12), (m, n, has)
                assert np.isnan(pts[:n][~ok]).all(), (m, n, has)
        # (the scene is ragged enough to matter: tracks with fewer than two, two, and more known views)
        seen = (full[..., 0] >= 0).sum(axis=1)
        assert (seen < 2).any() and (seen == 2).any() and (m < 4 or (seen > 2).any())


def test_triangulate_tracks_rejects_zero_and_nine_views(gpu_device):
    tracks = np.zeros((4, 9, 2), dtype=np.int32)
    P, has = np.zeros((9, 3, 4)), np.ones(9, dtype=np.uint8)
    for m, code in ((0, -1), (9, -3)):  # CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED
        rc, pts, ok = _triangulate(gpu_device, tracks, m, P, has)
        assert rc == code and b"1 to 8 images" in _lib.lib().cvhip_last_error()
        assert (pts == -5.0).all() and (ok == 9).all()


@pytest.mark.parametrize("m,image,placed", pc.MULTIVIEW_CONFIGS)
def test_pose_models_match_restatement_at_every_view_count(gpu_device, m, image, placed):
    """test_pose_models_match_restatement_per_sample's comparison (pose_checks.check_models, the same rules and bounds)
    with the image first, in the middle and last, 2 to m - 1 known views, m in {3, 4, 6, 8}.  The image's own slot is the
    candidate's: has_projection[image] = 1 with any matrix there changes no bit of the outputs."""
    tracks, K, P, has, projections = pc.multiview_config(m, image, placed)
    rc, pts, ok = _triangulate(gpu_device, tracks, m, P, has)
    assert rc == 0
    ok = ok.astype(bool)
    lt, lp = rp.linked(tracks, pts, ok, image)
    samples = pc.sample_triples(lp, pc.MULTIVIEW_TRIPLES)
    got = pc.device_models(gpu_device, tracks, pts, ok, P, has, image, K, 512, samples)
    pc.check_models(got, lt, lp, projections, image, K, 512, samples, label=f"m={m} image={image} known={placed}: ")
    P2, has2 = P.copy(), has.copy()
    P2[image] = np.arange(12.0).reshape(3, 4) - 3.5
    has2[image] = 1
    again = pc.device_models(gpu_device, tracks, pts, ok, P2, has2, image, K, 512, samples)
    for a, b in zip(got, again):
        assert np.array_equal(a, b, equal_nan=True)


def _compare_run(got, want_count, want_error, want_batches, want_winner, r, t, P):
    assert got["winner"] == tuple(want_winner) and got["count"] == want_count and got["batches"] == want_batches
    assert np.isclose(got["error"], want_error, rtol=1e-9, atol=0)
    assert np.allclose(got["r"], r, rtol=1e-9, atol=1e-12) and np.allclose(got["t"], t, rtol=1e-9, atol=1e-12)
    assert np.allclose(got["projection"], P, rtol=1e-9, atol=1e-9)


def _run_inputs(name):
    """pose_checks.run_inputs (the fixture generator's inputs: both sides get the restatement's points) in the device's form."""
    tracks, pts, ok, projections, image, K, md, seed = pc.run_inputs(name)
    has = np.array([pr is not None for pr in projections], dtype=np.uint8)
    P = np.ascontiguousarray(np.stack([pr if pr is not None else np.zeros((3, 4)) for pr in projections]))
    return tracks, K, P, has, image, pts, ok, md, seed, projections


def test_recover_pose_leaves_in_a_middle_batch(gpu_device):
    """cvhip_recover_pose on the middle-batch run against a live ref_pose.recover_pose: the carried result is replaced in
    batch 1, kept through batch 2 and replaced again in batch 3, after which the run leaves."""
    tracks, K, P, has, image, pts, ok, md, seed, projections = _run_inputs("middle_batch")
    rc, a = pc.device_recover_pose(gpu_device, tracks, pts, ok, P, has, image, K, md, seed)
    rc2, b = pc.device_recover_pose(gpu_device, tracks, pts, ok, P, has, image, K, md, seed)
    assert rc == 0 and rc2 == 0
    assert all(np.array_equal(a[k], b[k]) for k in a)
    want = rp.recover_pose(tracks, pts, ok, projections, image, K, md, seed)
    print("middle batch: device", a["winner"], a["count"], a["batches"], "restated", want["winner"], want["count"],
          want["batches"], "of", want["linked"])
    assert want["camera"] is not None and 2 <= want["batches"] <= 20 and want["winner"][0] >= 1
    _compare_run(a, want["count"], want["error"], want["batches"], want["winner"], *want["camera"])


def _fixture(name):
    return json.loads(GOLDEN.read_text())["runs"][name]


@pytest.mark.parametrize("name", ["accepted_late", "scrambled_rejected", "stage_scrambled"])
def test_recover_pose_all_batches_matches_fixture(gpu_device, name):
    """All 100 batches, accepted with a winner in a late batch, and rejected (CVHIP_ERR_NO_SURFACE, the best found still
    reported; once on the known scene, once on the restated sparse stage's table with the first two cameras recovered),
    against the restatement's recorded run; the winner's own hypothesis is re-derived live."""
    fx = _fixture(name)
    tracks, K, P, has, image, pts, ok, md, seed, projections = _run_inputs(name)
    assert md == fx["max_dimension"] and fx["batches"] == 100 and pc.table_digest(tracks) == fx["table"]
    assert image == fx["image"] and seed == fx["seed"]
    rc, a = pc.device_recover_pose(gpu_device, tracks, pts, ok, P, has, image, K, md, seed)
    rc2, b = pc.device_recover_pose(gpu_device, tracks, pts, ok, P, has, image, K, md, seed)
    print(name, "device", rc, a["winner"], a["count"], a["batches"], "fixture", fx["winner"], fx["count"], "of", fx["linked"])
    assert rc == rc2 and all(np.array_equal(a[k], b[k]) for k in a)
    if fx["accepted"]:
        assert rc == 0 and fx["count"] > fx["ransac_d"]
    else:
        assert rc == -6 and b"Unable to find projection matrix" in _lib.lib().cvhip_last_error()
        assert fx["count"] <= fx["ransac_d"]
    _compare_run(a, fx["count"], fx["error"], 100, fx["winner"], fx["r"], fx["t"], fx["projection"])
    lt, lp = rp.linked(tracks, pts, ok, image)
    assert len(lt) == fx["linked"]
    batch, h, slot = fx["winner"]
    cands = rp.pose_candidates(lt, lp, projections, image, K, md, rp.device_samples(seed, batch, h, len(lt)))
    (w,) = [c for c in cands if c[0] == slot]
    assert w[5] and w[6] == a["count"]
    _compare_run(a, w[6], w[7], 100, fx["winner"], w[3], w[2], w[4])


# ---- the sparse stage from planted matches ----------------------------------------------------------------------------
class _Recording(triangulation.PerspectiveTriangulation):
    """Keeps the seed of every recover_next_cameras call, the state after it, and the table the stage ended with."""

    def recover_next_cameras(self, device, seed=0, progress=None):
        self.__dict__.setdefault("seeds", []).append(seed)
        try:
            return super().recover_next_cameras(device, seed=seed, progress=progress)
        finally:
            self.__dict__.setdefault("states", []).append((self.points.copy(), self.points_ok.copy(),
                                                          list(self.projections), list(self.cameras)))

    def complete_sparse_triangulation(self):
        self.sparse_table = self.tracks.copy()
        super().complete_sparse_triangulation()


def _stage_scene(name):
    if name == "equal_counts_4":
        return pose_scenes.equal_counts_scene()
    if name == "few_links_5":
        return pose_scenes.few_links_scene()
    if name == "scrambled_5":
        return pose_scenes.scrambled_scene()
    if name == "mixed_4":
        return pose_scenes.sparse_mixed_scene()
    tracks, K, poses, X = pose_scenes.multiview_scene(8, 260, seed=11, miss=0.3)
    return tracks, K, poses, X, pose_scenes.planted_matches(tracks, K, poses)


def _recorded_failure(tracks, points, ok, projections, image, K, max_dimension, seed):
    """Stands in for ref_pose.recover_pose in the restated stage: the scrambled image's 100 batches come from the fixture
    (after a check that it was recorded on these inputs), every other call is restated live."""
    fx = _fixture("stage_scrambled")
    if image != fx["image"]:
        return rp.recover_pose(tracks, points, ok, projections, image, K, max_dimension, seed)
    assert pc.table_digest(tracks) == fx["table"] and len(rp.linked(tracks, points, ok, image)[0]) == fx["linked"]
    assert seed == fx["seed"] and max_dimension == fx["max_dimension"] and not fx["accepted"]
    return {"camera": None, "best": (np.array(fx["r"]), np.array(fx["t"]), np.array(fx["projection"])), "count": fx["count"],
            "error": fx["error"], "batches": fx["batches"], "winner": tuple(fx["winner"]), "linked": fx["linked"],
            "ransac_d": fx["ransac_d"], "history": fx["history"]}


def _run_stage(dev, oracle, name, bundle_adjustment, seed=3):
    """The device's sparse stage and the restated one on the same planted matches, compared call by call.
    -> (tri, st, order, info)."""
    scene = _stage_scene(name)
    tracks, K, poses, _, matches = scene[:5]
    m = tracks.shape[1]
    shapes = scene[5] if len(scene) > 5 else [(512, 512)] * m  # (mixed_4: a size and a K per image)
    calibration = K if isinstance(K, list) else [K] * m
    tri = _Recording(m, shapes, bundle_adjustment=bundle_adjustment, calibration=calibration)
    st = rp.SparseTriangulation(m, shapes, calibration, oracle.extend_tracks)
    want_pairs = pose_scenes.restated_pairs(st, matches)
    for (i, j), (rows, F) in sorted(matches.items()):
        p2, score = tri.add_image_pair_sparse(dev, i, j, F, rows)
        wp2, wscore = want_pairs[(i, j)]
        assert score == wscore and np.allclose(p2, wp2, rtol=1e-9, atol=1e-9), (i, j)
    assert np.array_equal(tri.tracks, st.tracks)
    assert tri.best_initial_pair == st.best[1]
    table = tri.tracks.copy()
    order, info = reconstruction.recover_camera_poses(dev, tri, seed=seed)
    worder, calls = rp.recover_camera_poses(st, seed=seed, recover=_recorded_failure if name == "scrambled_5" else None)
    print(name, "order", order, "restated", worder, [(c["image"], c["pose"] and (c["pose"]["linked"], c["pose"]["count"],
                                                                              c["pose"]["batches"])) for c in calls])
    assert order == worder and len(info) == len(calls)
    assert tri.seeds == [seed + k for k in range(len(calls) + 1)]  # one per call, failed ones included, and the empty one
    assert np.array_equal(tri.sparse_table, table)
    for k, (got, want) in enumerate(zip(info, calls)):
        pts, ok, projections, cameras = tri.states[k]
        assert ("failure" in got) == ("failure" in want) and ("images" in got) != ("failure" in got), k
        if "failure" in got:
            assert "Unable to find projection matrix" in got["failure"] and got["image"] == want["image"]
        else:
            assert got["images"] == want["images"]
        if want["pose"] is not None:
            w = want["pose"]
            assert got["image"] == want["image"] and got["linked"] == w["linked"] == want["counts"][want["image"]], k
            assert got["count"] == w["count"] and got["batches"] == w["batches"], k
            assert got["winner"] == (tuple(w["winner"]) if w["winner"] else (-1, -1, -1)), k
        for i in range(m):
            assert (projections[i] is None) == (want["projections"][i] is None), (k, i)
            if projections[i] is None:
                continue
            assert np.allclose(projections[i], want["projections"][i], rtol=1e-9, atol=1e-9), (k, i)
            assert np.allclose(cameras[i][1], want["cameras"][i].r, rtol=1e-9, atol=1e-12), (k, i)
            assert np.allclose(cameras[i][2], want["cameras"][i].t, rtol=1e-9, atol=1e-12), (k, i)
        assert np.array_equal(ok, want["ok"]), k
        assert np.allclose(pts[ok], want["points"][ok], rtol=1e-9, atol=1e-12), k
    tri.tracks = table  # (the dense stage would refill the table; the sparse one stands in for it)
    return tri, st, order, info, calls


@pytest.mark.parametrize("name", ["equal_counts_4", "few_links_5", "scrambled_5", "ragged_8", "mixed_4"])
def test_sparse_stage_from_planted_matches(gpu_device, oracle, name):
    """add_image_pair_sparse for every pair, reconstruction.recover_camera_poses and triangulate_all_recovered (no bundle
    adjustment) against ref_pose.SparseTriangulation / recover_camera_poses and
    ref_triangulation.triangulate_and_filter on the restated cameras: per pair the score and p2, the table bit for bit,
    the initial pair, the order, per call the image, linked, winner, count, batches, cameras, projections, points_ok and
    points; then the same kept set and points.  equal_counts_4: images 0 and 1 tie and the later one is taken.
    few_links_5: image 3's call fails at once, appears in the info and takes a seed; the image is pruned from the surface.
    scrambled_5: image 3 is tried first, fails after 100 batches (its restated run is tests/golden/pose_runs.json's
    stage_scrambled), and images 0 and 1 are placed after it with the next seeds.
    mixed_4 (pose_scenes.sparse_mixed_scene): a K and a (width, height) per image, landscape and portrait, only image 2
    past 1000 pixels - find_projection_matrix gets k1, k2 = the pair's own, recover_pose the image's own K and longer
    side, extend_tracks image 1's (width, height) for its grid and image 2's longer side for its radius, which is 4 for
    the pairs that end in image 2 and 3 for the others; tests/test_pose_ref.py shows that the table changes when the
    radius comes from the other image."""
    tri, st, order, info, calls = _run_stage(gpu_device, oracle, name, bundle_adjustment=False)
    m = tri.images_count
    if name == "equal_counts_4":
        first = calls[1]
        assert first["counts"][0] == first["counts"][1] and info[1]["image"] == 1 and order == [2, 3, 1, 0]
    keep = [i for i in range(m) if st.projections[i] is not None]
    if name == "few_links_5":
        assert "failure" in info[-1] and info[-1]["image"] == 3 and info[-1]["linked"] < rp.RANSAC_N
        assert info[-1]["batches"] == 0 and keep == [0, 1, 2, 4] and 3 not in order
    elif name == "scrambled_5":
        failed, fx = info[1], _fixture("stage_scrambled")
        assert "failure" in failed and failed["image"] == 3 and failed["batches"] == 100 and order == [2, 4, 0, 1]
        assert [p.get("images") for p in info[2:]] == [[0], [1]] and keep == [0, 1, 2, 4]
        _compare_run(failed, fx["count"], fx["error"], 100, fx["winner"], fx["r"], fx["t"], fx["projection"])
    else:
        assert keep == list(range(m)) and all(p["batches"] == 1 for p in info[1:])
    surf = tri.triangulate_all_recovered(gpu_device)
    assert len(surf.cameras) == len(keep) and surf.tracks.shape[1] == len(keep)
    table = tri.tracks[:, keep]
    idx, pts = rt.triangulate_and_filter(table, [st.cameras[i] for i in keep], [st.projections[i] for i in keep])
    assert np.array_equal(surf.track_index, idx) and len(idx) > 100
    assert np.array_equal(surf.tracks, table[idx])
    assert np.allclose(surf.points, pts, rtol=1e-9, atol=1e-12)


def test_sparse_stage_bundle_adjustment_matches_restatement(gpu_device, oracle):
    """The four-image stage with bundle adjustment, at the tolerances of
    test_reconstruct_perspective_512_bundle_adjustment_matches_restatement: the same kept set and accept / reject
    history, the final residual norm to 1e-6, points and cameras to 1e-4."""
    tri, st, order, info, calls = _run_stage(gpu_device, oracle, "equal_counts_4", bundle_adjustment=True)
    surf = tri.triangulate_all_recovered(gpu_device)
    cams = [st.cameras[i].copy() for i in range(4)]
    idx, pts = rt.triangulate_and_filter(tri.tracks, cams, st.projections)
    ba = rt.BundleAdjustment(cams, np.asarray(tri.tracks)[idx], pts)
    rcams = ba.optimize()
    print("bundle adjustment over 4 recovered cameras:", len(idx), "points,", len(ba.history), "iterations")
    assert np.array_equal(surf.track_index, idx)
    assert surf.ba_history == [int(h) for h in ba.history] and len(ba.history) > 0
    assert abs(surf.ba_residual_norms[1] - ba.final_residual_norm) <= 1e-6 * ba.final_residual_norm
    rel = np.linalg.norm(surf.points - ba.points, axis=1) / np.linalg.norm(ba.points, axis=1)
    assert (rel <= 1e-4).all(), rel.max()
    for dc, rc in zip(surf.cameras, rcams):
        assert np.allclose(dc.r, rc.r, rtol=1e-4, atol=1e-12) and np.allclose(dc.t, rc.t, rtol=1e-4, atol=1e-12)


# ---- a K per image, images of different shapes (tests/mixed_scenes.py) -----------------------------------------------------
@pytest.mark.parametrize("m,image,placed", pc.MIXED_CONFIGS)
def test_pose_models_match_restatement_on_mixed_cameras(gpu_device, m, image, placed):
    """test_pose_models_match_restatement_at_every_view_count's comparison (pose_checks.check_models as it is) where
    every image has its own K and its own (width, height): the known views' projections use their own K, the recovered
    image's K is its own, and max_dimension is that image's longer side, which is not its shorter one."""
    tracks, Ks, P, has, projections, sizes = pc.multiview_config_mixed(m, image, placed)
    size = max(sizes[image])
    assert size != min(sizes[image])
    rc, pts, ok = _triangulate(gpu_device, tracks, m, P, has)
    assert rc == 0
    ok = ok.astype(bool)
    lt, lp = rp.linked(tracks, pts, ok, image)
    samples = pc.sample_triples(lp, pc.MULTIVIEW_TRIPLES)
    got = pc.device_models(gpu_device, tracks, pts, ok, P, has, image, Ks[image], size, samples)
    pc.check_models(got, lt, lp, projections, image, Ks[image], size, samples, label=f"mixed m={m} image={image} known={placed}: ")


def test_recover_pose_whole_call_on_mixed_cameras(gpu_device):
    """cvhip_recover_pose, one whole call, on the mixed configuration (6, 3, (0, 1, 5)) - image 3 is 256 x 384 with its own
    K - against ref_pose.recover_pose on the same inputs (both sides get the restatement's points), compared as
    test_recover_pose_leaves_in_a_middle_batch compares: winner (batch, hypothesis, root), count, batches; error, r, t and
    projection to 1e-9.  The run leaves after batch 0 with at least 95 % of the linked tracks.  A second call gives the
    same bits."""
    tracks, K, P, has, image, pts, ok, md, seed, projections = pc.mixed_run_inputs()
    rc, a = pc.device_recover_pose(gpu_device, tracks, pts, ok, P, has, image, K, md, seed)
    rc2, b = pc.device_recover_pose(gpu_device, tracks, pts, ok, P, has, image, K, md, seed)
    assert rc == 0 and rc2 == 0
    assert all(np.array_equal(a[k], b[k]) for k in a)
    want = rp.recover_pose(tracks, pts, ok, projections, image, K, md, seed)
    print("mixed whole call: device", a["winner"], a["count"], a["batches"], "restated", want["winner"], want["count"],
          want["batches"], "of", want["linked"])
    assert want["camera"] is not None and want["batches"] == 1
    assert want["count"] >= rp.RANSAC_D_PERCENT_EARLY_EXIT * want["linked"] / 100 and want["linked"] > 300
    _compare_run(a, want["count"], want["error"], want["batches"], want["winner"], *want["camera"])
