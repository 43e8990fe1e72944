"""cybervision_amd/csrc/tiff_common.hpp as plain C++ on the CPU: tests/cpp/tiff_host.cpp, its own executable built with
AddressSanitizer and UBSan, against tests/ref_tiff.py's parse (the frame, the strip table, the EXIF focal length, the SEM
block), the SEM table against ref_tiff.sem_bytes, and over every truncation of two files and 400 seeded corruptions of
each: OK, INVALID or UNSUPPORTED comes back, never a sanitizer report."""
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_tiff
import tiff_scenes

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/tiff_host.cpp")
    out = tmp_path_factory.mktemp("tiff_host") / "tiff_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "tiff_host.cpp")])
    return out


def _run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return res.stdout.strip().splitlines()[-1]


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _sem(found, sw, sh, tilt, databar):
    return {"sem": found, "scale": [_bits(sw), _bits(sh)], "tilt": -1 if tilt is None else _bits(tilt), "databar": databar}


def _want(data):
    h = ref_tiff.parse(data)
    return {"code": 0, "width": h["width"], "height": h["height"], "samples": h["samples"], "bits": h["bits"], "compression": h["compression"],
            "photometric": h["photometric"], "predictor": h["predictor"], "rows_per_strip": h["rows_per_strip"], "focal": h["focal_length_35mm"],
            "little": h["order"] == "little", "row_bytes": h["row_bytes"], "strips": [list(t) for t in zip(h["offsets"], h["counts"], h["rows"])],
            **_sem(h["sem"], h["scale"][0], h["scale"][1], h["tilt_angle"], h["databar_height"])}


def test_parse_is_the_restated_parse(exe, tmp_path):
    for name in tiff_scenes.names():
        data = tiff_scenes.scene(name)
        (tmp_path / "in.tif").write_bytes(data)
        assert json.loads(_run(exe, "parse", tmp_path / "in.tif")) == _want(data), name


def test_refused_headers(exe, tmp_path):
    """The files the header refuses get the restatement's code; those only the decompression refuses parse."""
    parsed = []
    for name, (data, code) in sorted(tiff_scenes.refused().items()):
        (tmp_path / "in.tif").write_bytes(data)
        try:
            ref_tiff.parse(data)
            want = 0
            parsed.append(name)
        except ref_tiff.TiffError as err:
            want = err.code
            assert want == code, name
        assert json.loads(_run(exe, "parse", tmp_path / "in.tif"))["code"] == want, name
    assert parsed == sorted(n for n in tiff_scenes.refused() if n.startswith(("i_lzw_", "i_pb_")))


def test_sem_blocks(exe, tmp_path):
    for name, raw, _want_tuple in tiff_scenes.SEM_BLOCKS:
        (tmp_path / "block.txt").write_bytes(raw)
        assert json.loads(_run(exe, "sem", tmp_path / "block.txt")) == _sem(True, *ref_tiff.sem_bytes(raw)), name
        data = tiff_scenes.sem_file(raw, 34683)
        (tmp_path / "in.tif").write_bytes(data)
        assert json.loads(_run(exe, "parse", tmp_path / "in.tif")) == _want(data), name
    a, b = b"[PrivateFei]\nDatabarHeight=3\n", b"[PrivateFei]\nDatabarHeight=4\n"
    S = tiff_scenes.sem_file
    for data in (S(a, 34682, second=(34683, tiff_scenes.ASCII, b)), S(a, 34682, second=(34683, tiff_scenes.BYTE, b)), S(a, 34682, typ=7), S(b"ab\0"),
                 tiff_scenes.patch_entry(S(a), 34682, 1 << 30)):
        (tmp_path / "in.tif").write_bytes(data)
        assert json.loads(_run(exe, "parse", tmp_path / "in.tif")) == _want(data)


def test_exif_blocks(exe, tmp_path):
    g = tiff_scenes.picture(4, 4)
    for short in (True, False):
        for order in "<>":
            data = tiff_scenes.write(g, order, exif_focal=50, exif_short=short)
            assert ref_tiff.info(data)["focal_length_35mm"] == 50
            (tmp_path / "in.tif").write_bytes(data)
            assert json.loads(_run(exe, "parse", tmp_path / "in.tif")) == _want(data)
    base = tiff_scenes.write(g, exif_focal=50)
    for where in (len(base) - 3, 1 << 31, 4):   # broken Exif pointers: none, as the restatement says
        data = tiff_scenes.patch_entry(base, 34665, where)
        (tmp_path / "in.tif").write_bytes(data)
        got = json.loads(_run(exe, "parse", tmp_path / "in.tif"))
        assert got == _want(data) and got["focal"] == 0


@pytest.mark.parametrize("name", ["o_sem_exif", "o_70_strips_lzw"])
def test_truncations_and_corruptions(exe, tmp_path, name):
    data = tiff_scenes.scene(name)
    (tmp_path / "in.tif").write_bytes(data)
    ok, invalid, unsupported = (int(v) for v in _run(exe, "fuzz", tmp_path / "in.tif", 7, 400).split())
    assert ok + invalid + unsupported == len(data) + 400
    assert invalid >= len(data) - 4   # every cut but those in the next-IFD pointer: the IFD lies at the file's end
    assert ok > 0
