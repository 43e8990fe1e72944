"""max_points through the perspective pipeline (reconstruct_perspective / reconstruct_perspective_mesh): the
512^2 scene's surface with max_points is the restatement's subset (tests/ref_subset.py) of the surface without it, byte for
byte, and the mesh stage runs on the subset."""
import numpy as np
import pytest

import ref_subset
from cybervision_amd import mesh, reconstruction, synth

pytestmark = pytest.mark.gpu
# reconstruct_perspective_mesh's keys without max_points (test_mesh_obj_gpu.py pins them)
TODAYS_KEYS = {"surface", "camera_order", "poses", "initial_pair", "sparse", "sparse_tracks", "tracks", "cameras", "projections",
               "pairs", "timings_ms", "mesh", "depth_image", "mesh_image_shapes"}


def test_reconstruct_perspective_mesh_with_max_points(gpu_device):
    size, max_points, seed = 512, 5000, 7
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    first = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3)
    assert "subset" not in first and "subset" not in first["timings_ms"]
    full = first["surface"]
    n = len(full.points)
    assert n > 20000
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=first["pairs"],
                                                      max_points=max_points, max_points_seed=seed,
                                                      triangulate=mesh.delaunay_device(gpu_device))
    rows = ref_subset.subset_rows(n, max_points, seed)
    idx = rows.astype(np.int64)
    surface = out["surface"]
    assert len(surface.points) == len(surface.tracks) == len(surface.track_index) == max_points
    assert surface.points.tobytes() == full.points[idx].tobytes()
    assert surface.tracks.tobytes() == full.tracks[idx].tobytes()
    assert surface.track_index.tobytes() == full.track_index[idx].tobytes()
    assert len(surface.cameras) == len(full.cameras)
    assert set(out) == TODAYS_KEYS | {"subset"} and set(out["timings_ms"]) >= {"subset", "triangulate", "mesh"}
    assert set(out["subset"]) == {"rows_in", "rows_out", "seed", "rows"}
    assert (out["subset"]["rows_in"], out["subset"]["rows_out"], out["subset"]["seed"]) == (n, max_points, seed)
    assert np.array_equal(out["subset"]["rows"], rows)
    polys = np.asarray(out["mesh"]["polygons"])
    assert len(polys) > 1000 and int(polys.max()) < max_points
    # max_points >= the surface's length: the first surface, unchanged
    whole = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=first["pairs"],
                                                   max_points=n, max_points_seed=seed)
    assert whole["subset"]["rows_out"] == n and np.array_equal(whole["subset"]["rows"], np.arange(n, dtype=np.uint64))
    assert whole["surface"].points.tobytes() == full.points.tobytes() and whole["surface"].tracks.tobytes() == full.tracks.tobytes()
    assert whole["surface"].track_index.tobytes() == full.track_index.tobytes()
