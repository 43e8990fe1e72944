"""tests/ref_delaunay.py - the restatement of cvhip_mesh_delaunay's result - against answers written by hand, and scipy
against it where scipy is there.  CPU only."""
import numpy as np
import pytest

import ref_delaunay as rd


def test_brute_triangle_both_orders():
    assert rd.as_set(rd.brute(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]))) == {(0, 1, 2)}
    assert rd.as_set(rd.brute(np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0]]))) == {(0, 2, 1)}


def test_brute_point_inside_a_triangle():
    xy = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [1.0, 1.0]])
    assert rd.as_set(rd.brute(xy)) == {(0, 1, 3), (1, 2, 3), (0, 3, 2)}


@pytest.mark.parametrize("case", range(4))
def test_brute_unit_square_fans_from_the_lowest_index(case):
    xy, faces = rd.unit_square_cases()[case]
    assert rd.as_set(rd.brute(xy)) == set(faces)
    assert rd.check(xy, faces) == [] and rd.as_set(rd.canonical(xy, faces)) == set(faces)
    other = [(1, 2, 3), (0, 1, 3)] if case == 0 else None  # the other diagonal: Delaunay too, but not the defined fan
    if other:
        assert rd.check(xy, other) == [] and rd.as_set(rd.canonical(xy, other)) == set(faces)


def test_brute_circle_of_twelve():
    """the 12 integer points of x^2 + y^2 = 50 in a shuffled order, three points outside: the 12-gon is one fan of 10
    faces from its lowest index"""
    xy = rd.circle50()
    on = [i for i in range(len(xy)) if xy[i, 0] ** 2 + xy[i, 1] ** 2 == 50.0]
    assert len(on) == 12
    f = rd.brute(xy)
    inside = [t for t in f.tolist() if set(t) <= set(on)]
    assert len(inside) == 10 and all(t[0] == min(on) for t in inside)
    ring = sorted(on, key=lambda i: np.arctan2(xy[i, 1], xy[i, 0]))
    s = ring.index(min(on))
    ring = ring[s:] + ring[:s]
    assert set(map(tuple, inside)) == {(ring[0], ring[i], ring[i + 1]) for i in range(1, 11)}
    assert rd.check(xy, f) == [] and rd.as_set(rd.canonical(xy, f)) == rd.as_set(f)
    # all 15 points: 2 k - 2 - h faces
    assert len(f) == 2 * 15 - 2 - len(rd.Points(xy).hull())


def test_check_rejects():
    xy = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 1.0], [0.0, 1.5], [1.0, 0.4]])
    good = rd.brute(xy)
    assert rd.check(xy, good) == []
    faces = good.tolist()
    assert rd.check(xy, faces[:-1]), "a missing face"
    assert rd.check(xy, [faces[0][::-1]] + faces[1:]), "a reversed face"
    assert rd.check(xy, faces + [faces[0]]), "a doubled face"
    assert rd.check(xy, [[faces[0][1], faces[0][2], faces[0][0]]] + faces[1:]), "a face that is not rotated"
    # a flipped diagonal on a convex quadrilateral that is not co-circular
    quad = np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 1.0], [0.0, 1.2]])
    want = rd.as_set(rd.brute(quad))
    flipped = {(0, 1, 2), (0, 2, 3)} if want == {(0, 1, 3), (1, 2, 3)} else {(0, 1, 3), (1, 2, 3)}
    assert rd.check(quad, sorted(want)) == [] and any("locally" in v for v in rd.check(quad, sorted(flipped)))
    # a duplicate's higher index as a vertex
    dup = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
    assert rd.as_set(rd.brute(dup)) == {(0, 1, 2)} and rd.check(dup, [(0, 1, 2)]) == []
    assert any("duplicate" in v for v in rd.check(dup, [(0, 3, 2)]))


def test_scipy_passes_on_random_points():
    spatial = pytest.importorskip("scipy.spatial")
    xy = np.random.default_rng(3).uniform(0.0, 320.0, (30, 2))
    f = rd.orient_faces(xy, spatial.Delaunay(xy).simplices)
    assert rd.check(xy, f) == [] and rd.as_set(f) == rd.as_set(rd.brute(xy)) == rd.as_set(rd.canonical(xy, f))


def test_scipy_passes_on_a_scene():
    spatial = pytest.importorskip("scipy.spatial")
    import mesh_scenes
    import ref_mesh

    _, xy = ref_mesh.camera_points(mesh_scenes.scene(3).surface, 0)
    f = rd.orient_faces(xy, spatial.Delaunay(xy).simplices)
    assert len(f) > 5000 and rd.check(xy, f) == [] and rd.as_set(rd.canonical(xy, f)) == rd.as_set(f)
