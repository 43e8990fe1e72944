"""reconstruct_perspective and reconstruct_perspective_surface with resident_tracks=True (the dense track table in device
memory from extend_tracks to the surface) against resident_tracks=False, the host-table path, on config 5 at
512^2 with the same seed.  Every stage is integer or f64 in a fixed order: every comparison is equality of bytes."""
import numpy as np
import pytest

from cybervision_amd import mesh, reconstruction, synth, triangulation

pytestmark = pytest.mark.gpu
SIZE = 512


@pytest.fixture(scope="module")
def scene(gpu_device):
    views, K, poses = synth.make_sfm_views(SIZE)
    steps = synth.optimal_scale_steps(SIZE, SIZE)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False, seed=3)
    return pyrs, K, poses, pairs


def _host(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _same(a, b):
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(_host(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_surfaces(res, ref):
    s, r = res["surface"], ref["surface"]
    assert hasattr(s.points, "data_ptr") and s.points.is_cuda and hasattr(s.tracks, "data_ptr") and s.tracks.is_cuda
    assert isinstance(s.track_index, np.ndarray) and isinstance(r.points, np.ndarray)
    assert len(r.points) > 10_000 or "subset" in ref
    assert _same(s.points, r.points) and _same(s.track_index, r.track_index) and _same(s.tracks, r.tracks)
    assert len(s.cameras) == len(r.cameras)
    for a, b in zip(s.cameras, r.cameras):
        assert _same(a.r, b.r) and _same(a.t, b.t) and _same(a.projection, b.projection)
    assert s.ba_iterations == r.ba_iterations and s.ba_history == r.ba_history
    assert np.array(s.ba_residual_norms).tobytes() == np.array(r.ba_residual_norms).tobytes()
    assert isinstance(res["tracks"], triangulation.DeviceTrackTable) and isinstance(ref["tracks"], np.ndarray)
    assert res["tracks"].rows == len(ref["tracks"]) and _same(res["tracks"].numpy(), ref["tracks"])
    assert res.get("merges") == ref.get("merges")
    if "subset" in ref:
        assert _same(res["subset"]["rows"], ref["subset"]["rows"]) and res["subset"]["rows_out"] == ref["subset"]["rows_out"]
    assert set(res["timings_ms"]) == set(ref["timings_ms"])


@pytest.mark.parametrize("merge_tracks,bundle_adjustment,max_points",
                         [(False, False, None), (True, False, None), (False, True, None), (True, True, None), (True, False, 5000)])
def test_reconstruct_perspective_resident_equals_host_table(gpu_device, scene, merge_tracks, bundle_adjustment, max_points):
    pyrs, K, _poses, pairs = scene
    kw = dict(bundle_adjustment=bundle_adjustment, seed=3, pairs_result=pairs, merge_tracks=merge_tracks, max_points=max_points,
              max_points_seed=11)
    ref = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, **kw)
    res = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, resident_tracks=True, **kw)
    try:
        _check_surfaces(res, ref)
        assert res["camera_order"] == ref["camera_order"] and res["initial_pair"] == ref["initial_pair"]
        assert _same(res["sparse_tracks"], ref["sparse_tracks"])
        for a, b in zip(res["cameras"], ref["cameras"]):
            assert (a is None) == (b is None) and (a is None or all(_same(x, y) for x, y in zip(a, b)))
        for a, b in zip(res["projections"], ref["projections"]):
            assert (a is None) == (b is None) and (a is None or _same(a, b))
        if max_points is not None:
            assert len(ref["surface"].points) == max_points
            # the mesh stage on the device-tensor surface equals the same calls on its host copy
            s = res["surface"]
            shapes = [(SIZE, SIZE)] * len(s.cameras)
            copy = triangulation.Surface(points=_host(s.points), track_index=s.track_index, tracks=_host(s.tracks), cameras=s.cameras)
            tri = mesh.delaunay_device(gpu_device)
            got, want = mesh.create(gpu_device, s, shapes, tri), mesh.create(gpu_device, copy, shapes, tri)
            assert len(want["polygons"]) > 1000
            assert _same(got["polygons"], want["polygons"]) and _same(got["camera"], want["camera"])
            assert got["per_camera"] == want["per_camera"]
            assert _same(mesh.ply(gpu_device, s, got["polygons"]), mesh.ply(gpu_device, copy, want["polygons"]))
    finally:
        res["tracks"].close()


def test_reconstruct_perspective_surface_resident_equals_host_table(gpu_device, scene):
    pyrs, K, poses, pairs = scene
    cams = [(K, R, t) for R, t in poses]
    kw = dict(bundle_adjustment=False, merge_tracks=True)
    ref = reconstruction.reconstruct_perspective_surface(gpu_device, pyrs, pairs, cams, **kw)
    res = reconstruction.reconstruct_perspective_surface(gpu_device, pyrs, pairs, cams, resident_tracks=True, **kw)
    try:
        _check_surfaces(res, ref)
    finally:
        res["tracks"].close()
