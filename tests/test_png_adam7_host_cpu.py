"""cybervision_amd/csrc/png_decode_common.hpp's parse(.., adam7 = true) as plain C++ on the CPU: tests/cpp/png_adam7_host.cpp,
its own executable built with AddressSanitizer and UBSan, against tests/ref_png_adam7.py's parse on every scene, the refused
ones included - the header, the pass table and `filtered` -, over every truncation of two files and 400 seeded corruptions of
each, and parse(.., false), which still refuses every interlaced file as not built."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

import png_adam7_scenes as scenes
import png_in_scenes
import ref_png_adam7 as ref

ROOT = Path(__file__).resolve().parent.parent
KEYS = ("width", "height", "row_bytes", "first_row", "offset", "x0", "y0", "log_dx", "log_dy")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/png_adam7_host.cpp")
    out = tmp_path_factory.mktemp("png_adam7_host") / "png_adam7_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "png_adam7_host.cpp")])
    return out


def _run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return res.stdout.strip().splitlines()


def _parse_all(exe, folder, files):
    paths = []
    for k, data in enumerate(files):
        paths.append(folder / ("%d.png" % k))
        paths[-1].write_bytes(data)
    lines = _run(exe, "parse", *paths)
    assert len(lines) == len(files)
    return [json.loads(line) for line in lines]


def _want(data):
    """What the restatement says of the file: its code alone, or everything the parser holds."""
    try:
        h = ref.parse(data)
    except ref.PngError as err:
        return {"code": err.code}
    return {"code": 0, "width": h["width"], "height": h["height"], "colour": h["colour"], "depth": h["depth"], "interlace": h["interlace"],
            "channels": h["channels"], "bpp": h["bpp"], "focal": h["focal_length_35mm"], "flags": h["flags"], "palette_entries": len(h["palette"]) // 3,
            "idat": len(h["idat"]), "passes": h["passes"], "pass_rows": h["pass_rows"], "filtered": h["filtered"],
            "pass_table": [[e[k] for k in KEYS] for e in h["pass_table"]]}


def test_parse_is_the_restated_parse(exe, tmp_path):
    names = scenes.names()
    for name, got in zip(names, _parse_all(exe, tmp_path, [scenes.scene(n) for n in names])):
        assert got.pop("plain") == ref.UNSUPPORTED, name   # parse(.., false) still refuses
        assert got == _want(scenes.scene(name)) and got["interlace"] == 1 and len(got["pass_table"]) == 7, name
    # files that are not interlaced: one entry, the whole image, and parse(.., false) reads them
    plain = [n for n in png_in_scenes.names() if n[0] in "sfx"]
    for name, got in zip(plain, _parse_all(exe, tmp_path, [png_in_scenes.scene(n) for n in plain])):
        assert got.pop("plain") == 0, name
        want = _want(png_in_scenes.scene(name))
        assert got == want and got["pass_table"] == [[want["width"], want["height"], got["pass_table"][0][2], 0, 0, 0, 0, 0, 0]], name


def test_refused_headers(exe, tmp_path):
    """The files the chunk walk refuses get the restatement's code - among them 65 536 columns or rows and the passes of 2^31
    bytes -; those only the device refuses parse."""
    items = sorted(scenes.refused().items())
    parsed = 0
    for (name, (data, code)), got in zip(items, _parse_all(exe, tmp_path, [data for _n, (data, _c) in items])):
        want = _want(data)
        assert want["code"] in (0, code), name
        parsed += want["code"] == 0
        plain = got.pop("plain")
        assert got == want, name
        if data[28] == 1:
            assert plain in (ref.UNSUPPORTED, ref.INVALID), name   # parse(.., false) reads no interlaced file
    assert parsed >= 7   # the stream's own errors, the filter bytes and the palette index
    # every refused file of the decoder that is not interlaced keeps its code under parse(.., true)
    items = sorted(png_in_scenes.refused().items())
    for (name, (data, code)), got in zip(items, _parse_all(exe, tmp_path, [data for _n, (data, _c) in items])):
        if name == "u_adam7":
            assert (got["code"], got["plain"]) == (0, ref.UNSUPPORTED)
        else:
            assert got["code"] == got["plain"] == _want(data)["code"], name


@pytest.mark.parametrize("name", ["x_exif", "k_pal_d2_9x9"])
def test_truncations_and_corruptions(exe, tmp_path, name):
    data = scenes.scene(name)
    (tmp_path / "in.png").write_bytes(data)
    ok, invalid, unsupported = (int(v) for v in _run(exe, "fuzz", tmp_path / "in.png", 7, 400)[-1].split())
    assert ok + invalid + unsupported == len(data) + 400
    assert invalid >= len(data)   # every cut: the IEND chunk lies at the file's end
    assert ok > 0                 # a corruption inside the IDAT data is the device's to find
