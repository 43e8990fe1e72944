"""tiff_common.hpp's extended walk (parse(.., extended = true)) as plain C++ on the CPU: tests/cpp/tiff_ext_host.cpp,
its own executable built with AddressSanitizer and UBSan, against tests/ref_tiff_ext.py's parse - the frame, the tile
geometry, the stream table with every stream's row bytes and top-left sample -, the refused headers, and over every truncation
of two files and 400 seeded corruptions of each: OK, INVALID or UNSUPPORTED comes back, never a sanitizer report."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_tiff
import ref_tiff_ext
import tiff_ext_scenes
import tiff_scenes

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/tiff_ext_host.cpp")
    out = tmp_path_factory.mktemp("tiff_ext_host") / "tiff_ext_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "tiff_ext_host.cpp")])
    return out


def _run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return res.stdout.strip().splitlines()[-1]


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _want(data):
    h = ref_tiff_ext.parse(data)
    n = h["strips"]
    return {"code": 0, "width": h["width"], "height": h["height"], "samples": h["samples"], "bits": h["bits"], "compression": h["compression"],
            "photometric": h["photometric"], "predictor": h["predictor"], "rows_per_strip": h["rows_per_strip"], "focal": h["focal_length_35mm"],
            "little": h["order"] == "little", "row_bytes": h["row_bytes"],
            "tile": [h["tile_width"], h["tile_length"], h["tiles_across"], h["tiles_down"]],
            "streams": [list(t) for t in zip(h["offsets"], h["counts"], h["rows"], [h["stream_row_bytes"]] * n, h["xs"], h["ys"])],
            "sem": h["sem"], "scale": [_bits(h["scale"][0]), _bits(h["scale"][1])], "tilt": -1 if h["tilt_angle"] is None else _bits(h["tilt_angle"]),
            "databar": h["databar_height"]}


def test_walk_is_the_restated_walk(exe, tmp_path):
    """Every Deflate and tiled scene, and every file of the strip reader's scenes."""
    for scenes in (tiff_ext_scenes, tiff_scenes):
        for name in scenes.names():
            data = scenes.scene(name)
            (tmp_path / "in.tif").write_bytes(data)
            assert json.loads(_run(exe, "parse", tmp_path / "in.tif")) == _want(data), name


def test_refused_headers(exe, tmp_path):
    """The files the header refuses get the restatement's code; those only the decompression refuses are walked.  The strip
    reader's refusals too: what it refuses for its tiles or its compression is another answer here, the rest the same."""
    for name, (data, code, header) in sorted(tiff_ext_scenes.refused().items()):
        (tmp_path / "in.tif").write_bytes(data)
        got = json.loads(_run(exe, "parse", tmp_path / "in.tif"))["code"]
        assert got == (code if header else 0), name
    changed = []
    for name, (data, code) in sorted(tiff_scenes.refused().items()):
        (tmp_path / "in.tif").write_bytes(data)
        try:
            ref_tiff_ext.parse(data)
            want = 0
        except ref_tiff.TiffError as err:
            want = err.code
        assert json.loads(_run(exe, "parse", tmp_path / "in.tif"))["code"] == want, name
        try:
            ref_tiff.parse(data)
            old = 0
        except ref_tiff.TiffError as err:
            old = err.code
        if old != want:
            changed.append(name)
    assert changed == ["u_compression_32946", "u_compression_8", "u_tiles"]   # walked (their streams are no zlib streams); strip tags beside tile tags


@pytest.mark.parametrize("name", ["t_sem", "s_70_strips"])
def test_truncations_and_corruptions(exe, tmp_path, name):
    data = tiff_ext_scenes.scene(name)
    (tmp_path / "in.tif").write_bytes(data)
    ok, invalid, unsupported = (int(v) for v in _run(exe, "fuzz", tmp_path / "in.tif", 7, 400).split())
    assert ok + invalid + unsupported == len(data) + 400
    assert invalid >= len(data) - 4   # every cut but those in the next-IFD pointer: the IFD lies at the file's end
    assert ok > 0
