"""cvhip_merge_tracks (merge_tracks, triangulation.rs:1421-1540) on the device against the numpy
restatement (tests/ref_merge.py): bit-exact rows, tracks and counts, and config 5 with merge_tracks=True."""
import ctypes as C

import numpy as np
import pytest

import merge_scenes
import ref_merge
import ref_triangulation as rt
from cybervision_amd import _lib, reconstruction, synth, triangulation
from test_pose_gpu import _similarity_error, _sparse_restatement, _truth_points

pytestmark = pytest.mark.gpu


def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def device_merge(dev, tracks, image_index, w, h, m=None, device_tensors=False):
    """One cvhip_merge_tracks call -> (rc, rows, table, stats); outputs sized for n, host or torch tensors."""
    tracks = np.ascontiguousarray(tracks, dtype=np.int32)
    n = len(tracks)
    m = tracks.shape[1] if m is None else m
    rows = np.zeros(max(n, 1), dtype=np.uint64)
    out = np.zeros((max(n, 1), tracks.shape[1], 2), dtype=np.int32)
    stats = np.zeros(4, dtype=np.uint64)
    out_n = C.c_uint64(0)
    if device_tensors:
        import torch

        t_in = torch.from_numpy(tracks.reshape(-1).copy() if n else np.zeros(1, np.int32)).cuda()
        t_rows = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
        t_out = torch.zeros(out.size, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = _lib.lib().cvhip_merge_tracks(dev.handle, _ptr(t_in) if n else None, n, m, image_index, w, h, _ptr(t_rows),
                                           _ptr(t_out), C.byref(out_n), _ptr(stats))
        rows = t_rows.cpu().numpy().view(np.uint64)
        out = t_out.cpu().numpy().reshape(out.shape)
    else:
        rc = _lib.lib().cvhip_merge_tracks(dev.handle, _ptr(tracks) if n else None, n, m, image_index, w, h, _ptr(rows),
                                           _ptr(out), C.byref(out_n), _ptr(stats))
    k = out_n.value
    return rc, rows[:k].astype(np.int64), out[:k], tuple(int(v) for v in stats)


def _check(dev, tracks, i, w, h, **kw):
    rc, rows, table, stats = device_merge(dev, tracks, i, w, h, **kw)
    assert rc == 0, _lib.lib().cvhip_last_error()
    want_rows, want_stats = ref_merge.merge_tracks(tracks, i, w, h)
    assert np.array_equal(rows, want_rows), (tracks.shape, i, w, h)
    assert np.array_equal(table, tracks[want_rows])
    assert stats == want_stats
    return rows, stats


@pytest.mark.parametrize("x4, want", [(25, [1, 4, 2]), (45, [4, 2])])
def test_worked_example(gpu_device, x4, want):
    t = merge_scenes.worked_table(x4)
    rc, rows, table, stats = device_merge(gpu_device, t, 0, *merge_scenes.WORKED_SHAPE)
    assert rc == 0
    assert rows.tolist() == want
    assert np.array_equal(table, t[want])
    assert stats == (4, 3, 3 - len(want), 2)


def test_random_tables_bit_exact(gpu_device):
    rng = np.random.default_rng(5)
    for m in range(2, 9):
        for i in (0, m - 1):
            for w, h in ((37, 23), (640, 480), (1500, 700), (300, 2100)):
                n = int(rng.integers(1, 3 * w * h // 4))
                cells = int(rng.integers(1, w * h + 1))
                _check(gpu_device, merge_scenes.random_table(rng, n, m, w, h, i, cells=cells), i, w, h)
    # no rows; rows, none of them in image i
    rows, stats = _check(gpu_device, np.zeros((0, 3, 2), dtype=np.int32), 1, 64, 64)
    assert len(rows) == 0 and stats == (0, 0, 0, 0)
    t = merge_scenes.random_table(rng, 5000, 3, 64, 64, 1, p_present=0.0)
    rows, stats = _check(gpu_device, t, 1, 64, 64)
    assert len(rows) == 0 and stats == (0, 0, 0, 0)


def test_4096_table_bit_exact(gpu_device):
    """16.7 M cells: 65536 cell blocks, far past the 1024 lanes of the block-count scan; 6 M tracks over 3 images."""
    rng = np.random.default_rng(7)
    t = merge_scenes.random_table(rng, 6_000_000, 3, 4096, 4096, 2)
    rows, stats = _check(gpu_device, t, 2, 4096, 4096)
    assert stats[2] > 0 and len(rows) > 1_000_000


def test_host_and_device_pointers_and_repeats(gpu_device):
    rng = np.random.default_rng(9)
    t = merge_scenes.random_table(rng, 200_000, 4, 1024, 768, 1, cells=150_000)
    a = device_merge(gpu_device, t, 1, 1024, 768)
    b = device_merge(gpu_device, t, 1, 1024, 768)
    c = device_merge(gpu_device, t, 1, 1024, 768, device_tensors=True)
    d = device_merge(gpu_device, t, 1, 1024, 768, device_tensors=True)
    for other in (b, c, d):
        assert other[0] == 0 and np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2]) and a[3] == other[3]
    # either output may be left out
    n = len(t)
    rows = np.zeros(n, dtype=np.uint64)
    out_n = C.c_uint64(0)
    assert _lib.lib().cvhip_merge_tracks(gpu_device.handle, _ptr(t), n, 4, 1, 1024, 768, _ptr(rows), None, C.byref(out_n),
                                         None) == 0
    assert np.array_equal(rows[:out_n.value].astype(np.int64), a[1])


def test_errors_leave_the_outputs_untouched(gpu_device):
    rng = np.random.default_rng(3)
    base = merge_scenes.random_table(rng, 1000, 3, 50, 40, 0)
    one_negative = base.copy()
    one_negative[17, 2] = (5, -1)
    outside = base.copy()
    outside[500, 0] = (50, 3)
    below = base.copy()
    below[3, 0] = (2, 40)
    big = np.full((4, 9, 2), -1, dtype=np.int32)
    cases = [(base, 3, 3, -1), (base, 0, 3, 0), (one_negative, 0, 3, -1), (outside, 0, 3, -1), (below, 0, 3, -1),
             (big, 0, 9, -3)]
    for t, i, m, code in cases:
        n = len(t)
        rows = np.full(n, 0xABABABAB, dtype=np.uint64)
        out = np.full(t.shape, 0x5A5A5A5A, dtype=np.int32)
        stats = np.full(4, 77, dtype=np.uint64)
        out_n = C.c_uint64(12345)
        rc = _lib.lib().cvhip_merge_tracks(gpu_device.handle, _ptr(t), n, m, i, 50, 40, _ptr(rows), _ptr(out),
                                           C.byref(out_n), _ptr(stats))
        assert rc == code, (i, m, rc)
        if code == 0:
            continue
        assert out_n.value == 12345 and (rows == 0xABABABAB).all() and (out == 0x5A5A5A5A).all() and (stats == 77).all()


def _capture_merges(monkeypatch):
    """Wraps PerspectiveTriangulation.merge_tracks: (image, table before, table after, counts) of every call."""
    seen = []
    merge = triangulation.PerspectiveTriangulation.merge_tracks

    def wrapped(self, device, image_index):
        before = self.tracks.copy()
        info = merge(self, device, image_index)
        seen.append((image_index, self.image_shapes[image_index], before, self.tracks.copy(), info))
        return info

    monkeypatch.setattr(triangulation.PerspectiveTriangulation, "merge_tracks", wrapped)
    return seen


def _check_merges(seen, out):
    """Every merge of the run against the restatement on the device's own pre-merge table."""
    for image, (w, h), before, after, info in seen:
        rows, stats = ref_merge.merge_tracks(before, image, w, h)
        assert np.array_equal(after, before[rows]), image
        assert (info["rows_in"], info["rows_out"]) == (len(before), len(rows))
        assert (info["present"], info["cells"], info["rejected"], info["empty_area"]) == stats
    assert [s[4] for s in seen] == out["merges"]
    assert np.array_equal(out["tracks"], seen[-1][3])


def _config5(size):
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    return [synth.box_pyramid(v, steps) for v in views], K


def test_reconstruct_perspective_512_merges_match_restatement(gpu_device, monkeypatch):
    """Config 5 at 512^2 without bundle adjustment: one merge per linked image, the last one included, each equal to the
    restatement on the device's own pre-merge table; the final table is what reconstruct_perspective returns, and the
    run without merge_tracks is what it was."""
    size = 512
    pyrs, K = _config5(size)
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False, seed=3)
    plain = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=pairs)
    assert "merges" not in plain and "merge" not in plain["timings_ms"]
    seen = _capture_merges(monkeypatch)
    out = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=pairs,
                                                 merge_tracks=True)
    assert [s[0] for s in seen] == sorted(out["camera_order"])
    _check_merges(seen, out)
    last = sorted(out["camera_order"])[-1]
    assert (out["tracks"][:, last, 0] >= 0).all()
    assert np.array_equal(out["surface"].tracks, out["tracks"][out["surface"].track_index])
    print("512^2 merges", out["merges"], "surface", len(out["surface"].points), "of", len(plain["surface"].points),
          "without merge")


def test_reconstruct_perspective_512_merge_bundle_adjustment_matches_restatement(gpu_device, oracle, monkeypatch):
    """bundle_adjustment=True and merge_tracks=True at 512^2: the merges as above, then the surface against
    ref_triangulation on the merged table at the tolerances of
    test_reconstruct_perspective_512_bundle_adjustment_matches_restatement."""
    size = 512
    pyrs, K = _config5(size)
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False, seed=3)
    seen = _capture_merges(monkeypatch)
    out = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=True, seed=3, pairs_result=pairs,
                                                 merge_tracks=True)
    _check_merges(seen, out)
    st, order = _sparse_restatement(oracle, out, K, size, 3)
    assert out["camera_order"] == order
    keep = [i for i in range(3) if st.projections[i] is not None]
    table = out["tracks"]
    surf = out["surface"]
    cams = [st.cameras[i].copy() for i in keep]
    idx, pts = rt.triangulate_and_filter(table, cams, [st.projections[i] for i in keep])
    ba = rt.BundleAdjustment(cams, np.asarray(table)[idx], pts)
    rcams = ba.optimize()
    assert np.array_equal(surf.track_index, idx)
    assert surf.ba_history == [int(h) for h in ba.history]
    assert abs(surf.ba_residual_norms[1] - ba.final_residual_norm) <= 1e-6 * ba.final_residual_norm
    rel = np.linalg.norm(surf.points - ba.points, axis=1) / np.linalg.norm(ba.points, axis=1)
    assert (rel <= 1e-4).all(), rel.max()
    for dc, rc in zip(surf.cameras, rcams):
        assert np.allclose(dc.r, rc.r, rtol=1e-4, atol=1e-12) and np.allclose(dc.t, rc.t, rtol=1e-4, atol=1e-12)


def test_reconstruct_perspective_surface_512_merges_match_restatement(gpu_device, monkeypatch):
    """reconstruct_perspective_surface with the true cameras and merge_tracks=True at 512^2: a merge after every view's
    pairs, each equal to the restatement on the device's own pre-merge table; the surface (no bundle adjustment) is
    ref_triangulation's on the merged table."""
    size = 512
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False)
    cams = [(K, R, t) for R, t in poses]
    seen = _capture_merges(monkeypatch)
    out = reconstruction.reconstruct_perspective_surface(gpu_device, pyrs, pairs, cams, bundle_adjustment=False,
                                                         merge_tracks=True)
    assert [s[0] for s in seen] == [0, 1, 2] and "merge" in out["timings_ms"]
    _check_merges(seen, out)
    ref_idx, ref_pts, _, _ = rt.triangulate_all(out["tracks"], cams, bundle_adjustment=False)
    surf = out["surface"]
    assert len(ref_idx) > 10_000 and np.array_equal(surf.track_index, ref_idx)
    assert np.allclose(surf.points, ref_pts, rtol=1e-9, atol=1e-9)


def _view0_depth_error(out, K, size):
    """The surface's depth error against synth after a similarity alignment, over the points whose track has a view-0
    pixel (the truth is built from that pixel) -> (errors, selected points, all points)."""
    surf = out["surface"]
    sel = surf.tracks[:, 0, 0] >= 0
    return _similarity_error(surf.points[sel], _truth_points(surf.tracks[sel], K, size)), int(sel.sum()), len(surf.points)


def test_reconstruct_perspective_2048_merge(gpu_device, monkeypatch):
    """Config 5 at 2048^2 with merge_tracks=True, no bundle adjustment: every merge bit-exact against the restatement;
    the surface's depth error against synth after a similarity alignment, over the points whose track has a view-0 pixel,
    with the run without merges on the same pairs measured the same way for comparison.  Bound: DESIGN.md 4.10."""
    size = 2048
    pyrs, K = _config5(size)
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False, seed=3)
    plain = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=pairs)
    seen = _capture_merges(monkeypatch)
    out = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=pairs,
                                                 merge_tracks=True)
    _check_merges(seen, out)
    assert len(seen) == 3
    i1, _ = out["initial_pair"]
    if i1 != 0:
        return  # (the truth is built in camera 0's frame)
    err, k, n = _view0_depth_error(out, K, size)
    perr, pk, pn = _view0_depth_error(plain, K, size)
    print(f"2048^2 merge: order {out['camera_order']}, merges {out['merges']}, timings {out['timings_ms']}; "
          f"median depth error over the points with a view-0 pixel: {np.median(err):.4f} (p90 {np.percentile(err, 90):.4f}, "
          f"{k} of {n} points) with merges, {np.median(perr):.4f} (p90 {np.percentile(perr, 90):.4f}, {pk} of {pn} points) "
          f"without")
    # measured 2.96 % median (p90 5.91 %); the limit is that value with a 1.5x margin
    assert np.median(err) < 0.045
