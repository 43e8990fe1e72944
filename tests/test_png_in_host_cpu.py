"""cybervision_amd/csrc/png_decode_common.hpp as plain C++ on the CPU: tests/cpp/png_in_host.cpp, its own executable built
with AddressSanitizer and UBSan, against tests/ref_png_in.py's parse (the frame, the IDAT table, the palette, the eXIf focal
length), and over every truncation of two files and 400 seeded corruptions of each: OK, INVALID or UNSUPPORTED comes back,
never a sanitizer report."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

import png_in_scenes
import ref_png_in

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/png_in_host.cpp")
    out = tmp_path_factory.mktemp("png_in_host") / "png_in_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "png_in_host.cpp")])
    return out


def _run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return res.stdout.strip().splitlines()[-1]


def _want(data):
    h = ref_png_in.parse(data)
    return {"code": 0, "width": h["width"], "height": h["height"], "colour": h["colour"], "depth": h["depth"], "interlace": h["interlace"],
            "channels": h["channels"], "bpp": h["bpp"], "row_bytes": h["row_bytes"], "focal": h["focal_length_35mm"], "flags": h["flags"],
            "palette": list(h["palette"]), "idat": [list(t) for t in h["idat"]]}


def test_parse_is_the_restated_parse(exe, tmp_path):
    for name in png_in_scenes.names():
        data = png_in_scenes.scene(name)
        (tmp_path / "in.png").write_bytes(data)
        assert json.loads(_run(exe, "parse", tmp_path / "in.png")) == _want(data), name
    for name, data in png_in_scenes.accepted().items():
        (tmp_path / "in.png").write_bytes(data)
        assert json.loads(_run(exe, "parse", tmp_path / "in.png")) == _want(data), name


def test_refused_headers(exe, tmp_path):
    """The files the chunk walk refuses get the restatement's code; those only the device refuses parse."""
    parsed = 0
    for name, (data, code) in sorted(png_in_scenes.refused().items()):
        (tmp_path / "in.png").write_bytes(data)
        try:
            ref_png_in.parse(data)
            want = 0
            parsed += 1
        except ref_png_in.PngError as err:
            want = err.code
            assert want == code, name
        assert json.loads(_run(exe, "parse", tmp_path / "in.png"))["code"] == want, name
    assert parsed >= 20   # the stream's own errors, the IDAT CRC, the filter byte and the palette index


@pytest.mark.parametrize("name", ["x_short_le", "s_pal2_trns"])
def test_truncations_and_corruptions(exe, tmp_path, name):
    data = png_in_scenes.scene(name)
    (tmp_path / "in.png").write_bytes(data)
    ok, invalid, unsupported = (int(v) for v in _run(exe, "fuzz", tmp_path / "in.png", 7, 400).split())
    assert ok + invalid + unsupported == len(data) + 400
    assert invalid >= len(data)   # every cut: the IEND chunk lies at the file's end
    assert ok > 0                 # a corruption inside the IDAT data is the device's to find
