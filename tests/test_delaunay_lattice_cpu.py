"""LatticePolicy (cybervision_amd/csrc/delaunay_common.hpp) as plain C++ on the CPU, star by star against
ExactPolicy: tests/cpp/delaunay_lattice_exact.cpp, its own executable built with AddressSanitizer and UBSan - a 64-bit
in-circle determinant would trip UBSan's signed-overflow check on the scaled sets.  And triangulation.affine_surface through
the restatement of the mesh stage."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lattice_sets
import ref_delaunay as rd
import ref_mesh

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/delaunay_lattice_exact.cpp")
    out = tmp_path_factory.mktemp("delaunay_lattice") / "delaunay_lattice_exact"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "delaunay_lattice_exact.cpp")])
    return out


def run(exe, tmp_path, xy, cells=None):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    xy.tofile(tmp_path / "points.bin")
    cmd = [str(exe), str(tmp_path / "points.bin"), str(tmp_path / "faces.bin")] + ([str(cells)] if cells is not None else [])
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]  # (1: a star's faces differ between the policies; UBSan and ASan abort)
    return json.loads(res.stdout.strip().splitlines()[-1]), np.fromfile(tmp_path / "faces.bin", dtype=np.uint32).reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(lattice_sets.SETS))
def test_lattice_policy_is_the_exact_policy(exe, tmp_path, name):
    xy = lattice_sets.SETS[name]()
    assert (xy == np.rint(xy)).all() and np.abs(xy).max() <= lattice_sets.LIMIT
    info, f = run(exe, tmp_path, xy)
    assert info["k"] == len(xy) and info["faces"] == len(f) > 0
    assert info["flagged"] == 0  # (no duplicates: the lattice policy finishes every star)
    P = rd.Points(xy)
    assert rd.check(P, f) == []
    assert rd.as_set(rd.canonical(P, f)) == rd.as_set(f) and len(rd.as_set(f)) == len(f)
    if len(xy) <= 40:
        assert rd.as_set(f) == rd.as_set(rd.brute(P))


def test_duplicates_leave_the_lattice_path(exe, tmp_path):
    """a star that meets a duplicate where it could choose the wrong index flags; every other star still emits the exact faces"""
    xy, n_dup = lattice_sets.with_duplicates()
    info, f = run(exe, tmp_path, xy)
    P = rd.Points(xy)
    assert int((P.vertex != np.arange(P.k)).sum()) == n_dup
    assert 2 * n_dup <= info["flagged"] < len(xy) // 2  # (at least both indices of every pair; far from every star)
    assert rd.check(P, f) == [] and rd.as_set(rd.canonical(P, f)) == rd.as_set(f)


# ---- triangulation.affine_surface ------------------------------------------------------------------------------------------------
def test_affine_surface_shapes_and_cameras():
    from cybervision_amd import triangulation

    pts, p2 = lattice_sets.affine_points(40, 30, 40)
    s = triangulation.affine_surface(pts, p2)
    n = len(pts)
    assert s.points.shape == (n, 3) and s.points.tobytes() == pts.tobytes()
    assert s.track_index.tolist() == list(range(n))
    assert s.tracks.shape == (n, 2, 2) and s.tracks.dtype == np.int32
    assert np.array_equal(s.tracks[:, 0], pts[:, :2].astype(np.int32)) and np.array_equal(s.tracks[:, 1], p2.astype(np.int32))
    assert len(s.cameras) == 2
    for c in s.cameras:
        assert c.r.tolist() == [0.0, 0.0, 0.0] and c.t.tolist() == [0.0, 0.0, 0.0]
        assert np.asarray(c.projection).tolist() == [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        triangulation.affine_surface(pts, p2[:-1])


def test_affine_surface_through_the_mesh_restatement(exe, tmp_path):
    """ref_mesh.create on a 40 x 30 surface with holes: the projections are the pixels, the depth is z, the culling keeps every
    polygon of both cameras (a Delaunay triangle holds no other point, and at a vertex pixel the interpolated depth is the
    vertex's own), and the merge leaves the shared triangles with camera 0"""
    from cybervision_amd import triangulation

    pts, p2 = lattice_sets.affine_points(40, 30, 40)
    dev = triangulation.affine_surface(pts, p2)
    s = ref_mesh.Surface.from_device(dev, [(40, 30), (40, 30)])
    for j in range(2):
        idx, xy = ref_mesh.camera_points(s, j)
        assert idx.tolist() == list(range(len(pts))) and xy.tobytes() == np.ascontiguousarray(pts[:, :2]).tobytes()
        assert s.depth(j).tobytes() == np.ascontiguousarray(pts[:, 2]).tobytes()
    _, faces = run(exe, tmp_path, pts[:, :2])
    polygons, camera, per = ref_mesh.create(s, lambda xy: faces)
    assert len(per) == 2
    for idx, polys, keep in per:
        assert len(polys) == len(faces) > 2 * len(pts) - 200 and keep.all()
    assert len(polygons) == len(faces) and (camera == 0).all()
    assert rd.as_set(polygons) == rd.as_set(faces)
