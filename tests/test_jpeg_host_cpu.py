"""cybervision_amd/csrc/jpeg_common.hpp as plain C++ on the CPU: tests/cpp/jpeg_host.cpp, its own executable built with
AddressSanitizer and UBSan, against tests/ref_jpeg.py's parse (the frame, the tables, the lookups, the scan's range, the
EXIF focal length), and over every truncation of two files and a few hundred seeded corruptions: OK, INVALID or
UNSUPPORTED comes back, never a sanitizer report."""
import json
import shutil
import subprocess
import zlib
from pathlib import Path

import pytest

import jpeg_scenes
import ref_jpeg

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/jpeg_host.cpp")
    out = tmp_path_factory.mktemp("jpeg_host") / "jpeg_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "jpeg_host.cpp")])
    return out


def _run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return res.stdout.strip().splitlines()[-1]


def _want(data):
    h = ref_jpeg.parse(data)
    comps = []
    for c in h["comps"]:
        comps.append({"id": c["id"], "h": c["h"], "v": c["v"], "tq": c["tq"], "td": c["td"], "ta": c["ta"], "quant": h["quant"][c["tq"]],
                      "dc_lut": zlib.crc32(h["huff"][(0, c["td"])]["lut"].astype("<u2").tobytes()),
                      "ac_lut": zlib.crc32(h["huff"][(1, c["ta"])]["lut"].astype("<u2").tobytes())})
    mcus = h["mcus_x"] * h["mcus_y"]
    return {"code": 0, "width": h["width"], "height": h["height"], "components": len(comps), "hmax": h["hmax"], "vmax": h["vmax"],
            "mcus_x": h["mcus_x"], "mcus_y": h["mcus_y"], "restart": h["restart"], "focal": h["focal_length_35mm"], "scan": list(h["scan"]),
            "segments": -(-mcus // h["restart"]) if h["restart"] else 1, "bpm": sum(c["h"] * c["v"] for c in h["comps"]), "comps": comps}


@pytest.mark.parametrize("name", jpeg_scenes.names())
def test_parse_is_the_restated_parse(exe, tmp_path, name):
    data = jpeg_scenes.scene(name)
    (tmp_path / "in.jpg").write_bytes(data)
    assert json.loads(_run(exe, "parse", tmp_path / "in.jpg")) == _want(data)


def test_refused_headers(exe, tmp_path):
    """The files the header refuses get the restatement's code; those only the entropy decode refuses parse."""
    for name, (data, code) in sorted(jpeg_scenes.refused().items()):
        (tmp_path / "in.jpg").write_bytes(data)
        try:
            ref_jpeg.parse(data)
            want = 0
        except ref_jpeg.JpegError as err:
            want = err.code
            assert want == code, name
        assert json.loads(_run(exe, "parse", tmp_path / "in.jpg"))["code"] == want, name


def test_exif_blocks(exe, tmp_path):
    base = jpeg_scenes.scene("e_exif")
    at = base.index(b"Exif\0\0")
    old = int.from_bytes(base[at - 2:at], "big") - 2 - 6
    for short in (True, False):
        for big in (True, False):
            block = jpeg_scenes.exif_bytes(50, short, big)
            data = base[:at - 2] + (len(block) + 8).to_bytes(2, "big") + b"Exif\0\0" + block + base[at + 6 + old:]
            assert ref_jpeg.info(data)["focal_length_35mm"] == 50
            (tmp_path / "in.jpg").write_bytes(data)
            assert json.loads(_run(exe, "parse", tmp_path / "in.jpg")) == _want(data)
    block = jpeg_scenes.exif_bytes(50)
    for cut in range(0, len(block), 3):   # broken blocks: none, as the restatement says
        data = base[:at - 2] + (cut + 8).to_bytes(2, "big") + b"Exif\0\0" + block[:cut] + base[at + 6 + old:]
        (tmp_path / "in.jpg").write_bytes(data)
        assert json.loads(_run(exe, "parse", tmp_path / "in.jpg"))["focal"] == ref_jpeg.info(data)["focal_length_35mm"]


@pytest.mark.parametrize("name", ["e_exif", "w_restart"])
def test_truncations_and_corruptions(exe, tmp_path, name):
    data = jpeg_scenes.scene(name)
    (tmp_path / "in.jpg").write_bytes(data)
    ok, invalid, unsupported = (int(v) for v in _run(exe, "fuzz", tmp_path / "in.jpg", 7, 400).split())
    assert ok + invalid + unsupported == len(data) + 400
    assert invalid >= ref_jpeg.parse(data)["scan"][0] - 1   # every cut inside the header
    assert ok > 0


def test_refusals_are_the_recorded_ones(exe, tmp_path):
    """Code and reason of every refused scene, and a CRC over the code and reason of every truncation and corruption in order,
    are those the walk gave before the two decoders shared it (tests/golden/jpeg_walk_reasons.json): a file with several
    defects is still refused for the same one."""
    golden = json.loads((ROOT / "tests" / "golden" / "jpeg_walk_reasons.json").read_text())["baseline"]
    scenes = jpeg_scenes.refused()
    assert sorted(scenes) == sorted(golden["refused"])
    for name, (data, _) in sorted(scenes.items()):
        (tmp_path / "in.jpg").write_bytes(data)
        got = json.loads(_run(exe, "parse", tmp_path / "in.jpg"))
        assert [got["code"], got.get("reason", "")] == golden["refused"][name], name
    for name, crc in sorted(golden["fuzz"].items()):
        (tmp_path / "in.jpg").write_bytes(jpeg_scenes.scene(name))
        res = subprocess.run([str(exe), "fuzz", str(tmp_path / "in.jpg"), "7", "400"], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
        assert res.stdout.strip().splitlines()[-2] == "reasons %d" % crc, name
