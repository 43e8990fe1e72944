"""tests/ref_obj.py against itself and against answers written by hand: the two forms of `{}` on the value set, the two forms
of the file image on the scenes of the device tests, and the rules a reader of ObjWriter would check first."""
import numpy as np
import pytest

import obj_scenes
import ref_obj
from ply_scenes import SCALE
from ref_obj import COLOR, PLAIN, TEXTURE


def test_two_forms_agree_on_the_value_set():
    values = obj_scenes.value_set()
    assert len(values) > 1_200_000
    for v in values.tolist():
        a = ref_obj.display_a(v)
        if a != ref_obj.display_b(v):
            pytest.fail(f"{v!r}: {a} against {ref_obj.display_b(v)}")
        if v == v and float(a) != v:
            pytest.fail(f"{v!r}: {a} does not read back")


def test_known_answers():
    show = ref_obj.display_a
    assert [show(v) for v in (1.0, 100.0, 0.1, 0.1 + 0.2, 1.0 / 3.0)] == ["1", "100", "0.1", "0.30000000000000004", "0.3333333333333333"]
    assert show(1e23) == "1" + "0" * 23 and len(show(1e23)) == 24
    assert show(1e21) == "1" + "0" * 21 and show(1e22) == "1" + "0" * 22
    assert show(1e-7) == "0.0000001" and len(show(1e-7)) == 9
    assert show(123456789012345680000.0) == "123456789012345680000"
    assert show(2.0 ** 53 - 1.0) == "9007199254740991" and show(2.0 ** 53 + 2.0) == "9007199254740994"
    assert show(5e-324) == "0." + "0" * 323 + "5" and len(show(5e-324)) == 326
    assert show(2.2250738585072014e-308) == "0." + "0" * 307 + "22250738585072014"
    assert show(1.7976931348623157e308) == "17976931348623157" + "0" * 292 and len(show(1.7976931348623157e308)) == 309
    assert [show(v) for v in (0.0, -0.0, float("inf"), float("-inf"), float("nan"), -float("nan"))] == ["0", "-0", "inf", "-inf", "NaN", "NaN"]
    assert show(-1.5) == "-1.5" and show(1.0 / 255.0) == "0.00392156862745098" and show(255.0 / 255.0) == "1"


def test_mtl_known_answer():
    want = (b"newmtl Textured0\nKa 0.2 0.2 0.2\nKd 0.8 0.8 0.8\nKs 1.0 1.0 1.0\nillum 2\nNs 0.000500\nmap_Ka out-0.png\nmap_Kd out-0.png\n\n"
            b"newmtl Textured1\nKa 0.2 0.2 0.2\nKd 0.8 0.8 0.8\nKs 1.0 1.0 1.0\nillum 2\nNs 0.000500\nmap_Ka out-1.png\nmap_Kd out-1.png\n\n")
    assert ref_obj.mtl_bytes("out", 2) == want == ref_obj.mtl_bytes_scalar("out", 2)
    assert ref_obj.mtl_bytes("out", 0) == b"" == ref_obj.mtl_bytes_scalar("out", 0)


def test_texture_five_known_answer():
    """Cameras 0, 2, 2, 1, 0 give four usemtl lines; track 1 has no point in camera 2, whose polygons name it; track 2's point in
    image 0 lies past it (u = 1.5)."""
    points, tracks, dims, polygons, camera, text = obj_scenes.texture_five()
    for fn in (ref_obj.obj_bytes, ref_obj.obj_bytes_scalar):
        assert fn(points, tracks, dims, TEXTURE, (1.0, 1.0, 1.0), polygons, camera, "five") == text
    assert text.count(b"usemtl") == 4 and b"vt 1.5 0.875\n" in text and ref_obj.obj_sections(text, TEXTURE) == [16, 97, 177, 142]
    assert sum(ref_obj.obj_sections(text, TEXTURE)) == len(text)
    # the other modes on the same surface: no header, no vt, no usemtl, plain indices
    plain = ref_obj.obj_bytes(points, tracks, None, PLAIN, (1.0, 1.0, 1.0), polygons, camera, "five")
    assert plain == ref_obj.obj_bytes_scalar(points, tracks, None, PLAIN, (1.0, 1.0, 1.0), polygons, camera, "five")
    assert plain.endswith(b"v 7 -8 9\nf 3 2 1\nf 4 3 2\nf 6 5 4\nf 2 1 6\nf 6 1 3\n") and plain.startswith(b"v 0 -0 0\nv 1 -0.5 -2\n")
    # a camera past the track's length takes all of the track's points (take(camera) past the end)
    far = ref_obj.obj_bytes(points, tracks, dims, TEXTURE, (1.0, 1.0, 1.0), polygons[:1], [7], "five")
    assert far == ref_obj.obj_bytes_scalar(points, tracks, dims, TEXTURE, (1.0, 1.0, 1.0), polygons[:1], [7], "five")
    assert far.endswith(b"usemtl Textured7\nf 3/8 2/6 1/4\n")


def test_zero_width_and_colour_rules():
    points = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    tracks = np.array([[[0, 3], [2, 1]], [[5, 0], [-1, -1]]], dtype=np.int32)
    got = ref_obj.obj_bytes(points, tracks, [(0, 4), (4, 0)], TEXTURE, (1.0, 1.0, 1.0), np.zeros((0, 3)), None, "z")
    assert got == ref_obj.obj_bytes_scalar(points, tracks, [(0, 4), (4, 0)], TEXTURE, (1.0, 1.0, 1.0), np.zeros((0, 3)), None, "z")
    assert got == b"mtllib z.mtl\nv 1 -2 3\nv 4 -5 6\nvt NaN 0.25\nvt 0.5 -inf\nvt inf 1\n"
    # Color: the first present point's pixel, and no colour when that point lies past its image
    images = [np.zeros((4, 4, 3), dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.uint8)]
    images[0][3, 0] = [255, 51, 1]
    want = b"v 1 -2 3 1 0.2 0.00392156862745098\nv 4 -5 6\n"
    for fn in (ref_obj.obj_bytes, ref_obj.obj_bytes_scalar):
        assert fn(points, tracks, images, COLOR, (1.0, 1.0, 1.0), np.zeros((0, 3)), None, "z") == want
    lost = tracks.copy()
    lost[1] = -1
    for fn in (ref_obj.obj_bytes, ref_obj.obj_bytes_scalar):
        for mode in (COLOR, TEXTURE):
            with pytest.raises(ref_obj.TrackHasNoImages):
                fn(points, lost, images, mode, (1.0, 1.0, 1.0), np.zeros((0, 3)), None, "z")
        assert fn(points, lost, None, PLAIN, (1.0, 1.0, 1.0), np.zeros((0, 3)), None, "z") == b"v 1 -2 3\nv 4 -5 6\n"


@pytest.mark.parametrize("mode", [PLAIN, COLOR, TEXTURE])
def test_two_forms_agree_on_the_scene(mode):
    points, tracks, polygons, camera, images = obj_scenes.scene()
    assert len(points) == 12288 and len(polygons) == 12941 + 12910 + 12526
    a = ref_obj.obj_bytes(points, tracks, images, mode, SCALE, polygons, camera, "scene")
    assert a == ref_obj.obj_bytes_scalar(points, tracks, images, mode, SCALE, polygons, camera, "scene")
    assert sum(ref_obj.obj_sections(a, mode)) == len(a)


def test_two_forms_agree_on_long_records():
    points, tracks, polygons, camera = obj_scenes.long_records()
    a = ref_obj.obj_bytes(points, tracks, None, PLAIN, (1.0, 1.0, 1.0), polygons, camera, "long")
    assert a == ref_obj.obj_bytes_scalar(points, tracks, None, PLAIN, (1.0, 1.0, 1.0), polygons, camera, "long")
    lines = a.split(b"\n")
    assert min(len(line) for line in lines[:256]) > 960 and sum(len(line) + 1 for line in lines[:256]) > 245_000
