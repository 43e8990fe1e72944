"""cvhip_mesh_delaunay on a real GPU against tests/ref_delaunay.py: `check` empty and `canonical` equal say
that the faces are THE defined result; scipy's triangulation, where scipy is there, must be the same set."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_scenes
import ref_delaunay as rd
import ref_mesh
from cybervision_amd import _lib, mesh, reconstruction, synth

pytestmark = pytest.mark.gpu
UNBOUNDED = mesh.LANE_CELLS_UNBOUNDED


@pytest.fixture(autouse=True)
def default_lane_cells(gpu_device):
    yield
    mesh.set_delaunay_lane_cells(gpu_device, mesh.DELAUNAY_LANE_CELLS_DEFAULT)


def defined(xy, faces):
    """`faces` are the defined result for xy -> the Points (for further questions)"""
    P = rd.Points(xy)
    f = np.asarray(faces, dtype=np.int64)
    assert rd.check(P, f) == []
    assert rd.as_set(rd.canonical(P, f)) == rd.as_set(f) and len(rd.as_set(f)) == len(f)
    return P


def scipy_set(xy):
    try:
        from scipy.spatial import Delaunay
    except ImportError:
        return None
    return rd.as_set(rd.orient_faces(xy, Delaunay(xy).simplices))


@functools.lru_cache(maxsize=None)
def scene_points(m, camera):
    return ref_mesh.camera_points(_scene(m).surface, camera)[1]


@functools.lru_cache(maxsize=None)
def _scene(m):
    return mesh_scenes.scene(m)


TINY = {
    "k0": np.zeros((0, 2)), "k1": np.array([[1.0, 2.0]]), "k2": np.array([[1.0, 2.0], [3.0, 1.0]]),
    "k3": np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), "k3_other_order": np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]]),
    "k3_collinear": np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]]),
    "k4_convex": np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 1.0], [0.0, 1.2]]),
    "k4_inner": np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [1.0, 1.0]]),
    "square0": rd.unit_square_cases()[0][0], "square1": rd.unit_square_cases()[1][0], "square2": rd.unit_square_cases()[2][0],
    "square3": rd.unit_square_cases()[3][0], "circle50": rd.circle50(),
}


@pytest.mark.parametrize("name", sorted(TINY))
def test_tiny(gpu_device, name):
    xy = TINY[name]
    stats = {}
    f = mesh.delaunay(gpu_device, xy, stats)
    assert f.dtype == np.uint32 and f.shape == (len(f), 3)
    assert rd.as_set(f) == rd.as_set(rd.brute(xy)) and len(rd.as_set(f)) == len(f)
    if name in ("k0", "k1", "k2", "k3_collinear"):
        assert len(f) == 0
    if name == "k3":
        assert f.tolist() == [[0, 1, 2]]
    if name == "k3_other_order":
        assert f.tolist() == [[0, 2, 1]]
    if name.startswith("square"):
        assert rd.as_set(f) == set(rd.unit_square_cases()[int(name[-1])][1])
    if len(xy) >= 3:
        assert stats["device_stars"] + stats["host_stars"] == len(xy)


@pytest.mark.parametrize("k", [255, 256, 257])
def test_block_edges(gpu_device, k):
    xy = np.random.default_rng(k).uniform(0.0, 320.0, (k, 2))
    f = mesh.delaunay(gpu_device, xy)
    defined(xy, f)
    want = scipy_set(xy)
    assert want is None or rd.as_set(f) == want


@pytest.mark.parametrize("m,camera", [(m, c) for m in (2, 3, 8) for c in range(m)])
def test_scene_cameras(gpu_device, m, camera):
    """The real shape: a jittered lattice, a random subset per camera, doubled density over the foreground - at the default
    lane_cells, 0 (every star on the exact host path), 16, 96 (mixed) and unbounded: one face set, and at the default the
    device does the work."""
    xy = scene_points(m, camera)
    k = len(xy)
    stats = {}
    f = mesh.delaunay(gpu_device, xy, stats)
    defined(xy, f)
    want = scipy_set(xy)
    assert want is None or rd.as_set(f) == want
    print(f"scene({m}) camera {camera}: {k} points, {len(f)} faces, stats {stats}")
    assert stats["device_stars"] + stats["host_stars"] == k and stats["duplicates"] == 0
    assert stats["host_stars"] <= k // 10
    rows = f[np.lexsort(f.T[::-1])]
    for cells in (0, 16, 96, UNBOUNDED):
        mesh.set_delaunay_lane_cells(gpu_device, cells)
        st = {}
        g = mesh.delaunay(gpu_device, xy, st)
        assert np.array_equal(g[np.lexsort(g.T[::-1])], rows), cells
        assert g.tobytes() == f.tobytes(), cells  # (the order is defined too)
        if cells == 0:
            assert st["device_stars"] == 0 and st["host_stars"] == k
        if cells in (16, 96):
            assert st["host_stars"] > stats["host_stars"]
        if cells == 96:
            assert 0 < st["device_stars"] < k  # (mixed: an interior star visits about 85 cells)


def test_past_one_launch(gpu_device):
    """a jittered 513 x 513 lattice: more points than CVHIP_MESH_GRID_LANES"""
    n = 513
    rng = np.random.default_rng(513)
    gy, gx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    xy = np.stack([gx.ravel() + rng.uniform(0.2, 0.8, n * n), gy.ravel() + rng.uniform(0.2, 0.8, n * n)], axis=1)
    assert len(xy) == 263169 > mesh.GRID_LANES
    stats = {}
    f = mesh.delaunay(gpu_device, xy, stats)
    P = defined(xy, f)
    assert len(f) == 2 * len(xy) - 2 - len(P.hull())
    print(f"513 x 513: {len(f)} faces, stats {stats}")
    assert stats["host_stars"] <= len(xy) // 10


def test_uneven_density(gpu_device):
    """1000 points in a disc of radius 1 and 1000 across [-1280, 1600)^2: over-full cells, empty cells, long stars"""
    rng = np.random.default_rng(77)
    d = rng.uniform(-1.0, 1.0, (4000, 2))
    d = d[(d ** 2).sum(axis=1) < 1.0][:1000]
    xy = np.concatenate([d, rng.uniform(-1280.0, 1600.0, (1000, 2))])
    assert len(xy) == 2000
    stats = {}
    f = mesh.delaunay(gpu_device, xy, stats)
    defined(xy, f)
    print(f"uneven: {len(f)} faces, stats {stats}")


EXACT = {"circle50": rd.circle50, "lattice": rd.lattice, "nearly_collinear": rd.nearly_collinear, "circle50_ulp": rd.circle50_ulp,
         "duplicates": lambda: rd.with_duplicates()[0]}


@pytest.mark.parametrize("name", sorted(EXACT))
@pytest.mark.parametrize("cells", [mesh.DELAUNAY_LANE_CELLS_DEFAULT, UNBOUNDED])
def test_exactness(gpu_device, name, cells):
    xy = EXACT[name]()
    mesh.set_delaunay_lane_cells(gpu_device, cells)
    stats = {}
    f = mesh.delaunay(gpu_device, xy, stats)
    P = defined(xy, f)
    if len(xy) <= 40:
        assert rd.as_set(f) == rd.as_set(rd.brute(P))
    assert stats["duplicates"] == int((P.vertex != np.arange(P.k)).sum()) == (rd.with_duplicates()[1] if name == "duplicates" else 0)
    if name == "lattice":
        assert stats["host_stars"] == len(xy)  # every star of an integer lattice meets a tie


def test_abi(gpu_device):
    import torch

    xy = np.ascontiguousarray(scene_points(3, 1))
    k = len(xy)
    L = _lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    n = C.c_uint64(0)
    assert L.cvhip_mesh_delaunay(gpu_device.handle, p(xy), k, None, 0, C.byref(n), None) == 0  # the sizing call
    nf = n.value
    assert 0 < nf <= 2 * k
    exact = np.zeros((nf, 3), dtype=np.uint32)
    assert L.cvhip_mesh_delaunay(gpu_device.handle, p(xy), k, p(exact), nf, C.byref(n), None) == 0 and n.value == nf
    roomy = np.full((2 * k, 3), 0xABABABAB, dtype=np.uint32)
    assert L.cvhip_mesh_delaunay(gpu_device.handle, p(xy), k, p(roomy), 2 * k, C.byref(n), None) == 0 and n.value == nf
    assert roomy[:nf].tobytes() == exact.tobytes() and (roomy[nf:] == 0xABABABAB).all()  # two calls, the same bytes
    assert exact.tobytes() == mesh.delaunay(gpu_device, xy).tobytes()
    small = np.full((nf - 1, 3), 0xABABABAB, dtype=np.uint32)
    assert L.cvhip_mesh_delaunay(gpu_device.handle, p(xy), k, p(small), nf - 1, C.byref(n), None) == -1  # CVHIP_ERR_INVALID
    assert (small == 0xABABABAB).all()
    for bad in (np.nan, np.inf, -np.inf):
        broken = xy.copy()
        broken[k // 2, 1] = bad
        untouched = np.full((2 * k, 3), 0xABABABAB, dtype=np.uint32)
        assert L.cvhip_mesh_delaunay(gpu_device.handle, p(broken), k, p(untouched), 2 * k, C.byref(n), None) == -1
        assert (untouched == 0xABABABAB).all()
        with pytest.raises(_lib.CvhipError):
            mesh.delaunay(gpu_device, broken)
    assert L.cvhip_mesh_delaunay(gpu_device.handle, p(xy), 2 ** 32 - 1, p(roomy), 2 * k, C.byref(n), None) == -3  # CVHIP_ERR_UNSUPPORTED
    # device pointers in and out
    ordinal = getattr(gpu_device, "ordinal", -1)
    where = torch.device("cuda", ordinal) if ordinal >= 0 else "cuda"
    d_xy = torch.from_numpy(xy).to(where)
    d_faces = torch.zeros((2 * k, 3), dtype=torch.int32, device=where)
    torch.cuda.synchronize()
    st = np.zeros(len(mesh.DELAUNAY_STATS), dtype=np.uint64)
    assert L.cvhip_mesh_delaunay(gpu_device.handle, C.c_void_p(d_xy.data_ptr()), k, C.c_void_p(d_faces.data_ptr()), 2 * k, C.byref(n),
                                 p(st)) == 0 and n.value == nf
    assert d_faces[:nf].cpu().numpy().view(np.uint32).tobytes() == exact.tobytes()
    assert int(st[2]) + int(st[3]) == k and int(st[0]) * int(st[1]) >= k // 4


def test_through_mesh_create(gpu_device):
    s = _scene(3)
    dev_surface = mesh_scenes.device_surface(s)
    seen = []

    def triangulate(xy):
        f = mesh.delaunay_device(gpu_device)(xy)
        seen.append((xy, f))
        return f

    got = mesh.create(gpu_device, dev_surface, s.image_dims, triangulate)
    assert len(seen) == 3 and len(got["polygons"]) > 5000
    for xy, f in seen:
        defined(xy, f)
    try:
        import scipy  # noqa: F401
    except ImportError:
        return
    want = mesh.create(gpu_device, dev_surface, s.image_dims, lambda xy: rd.orient_faces(xy, mesh.delaunay_scipy(xy)))
    assert np.array_equal(got["polygons"], want["polygons"]) and np.array_equal(got["camera"], want["camera"])


def test_reconstruct_perspective_mesh_on_the_device(gpu_device, tmp_path):
    """Config 5's scene at 512^2 through reconstruct_perspective_mesh with the device's triangulator - no scipy anywhere"""
    size = 512
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    seen = []
    tri = mesh.delaunay_device(gpu_device)

    def triangulate(xy):
        seen.append((xy, tri(xy)))
        return seen[-1][1]

    path = tmp_path / "surface.ply"
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, triangulate=triangulate, project_to_image=0,
                                                      bundle_adjustment=False, seed=3, ply_path=str(path))
    assert len(out["surface"].cameras) == 3 and len(seen) == 3 and len(out["mesh"]["polygons"]) > 20000
    assert path.stat().st_size == sum(out["ply_sections"]) and out["ply_sections"][2] == 13 * len(out["mesh"]["polygons"])
    for xy, f in seen:
        assert len(f) > 10000
        defined(xy, f)
