"""cybervision_amd/csrc/jpeg_prog_common.hpp as plain C++ on the CPU: tests/cpp/jpeg_prog_host.cpp, its own executable built
with AddressSanitizer and UBSan, against tests/ref_jpeg_prog.py (the frame, the scan list, the lookups, the restart
intervals' byte ranges, and - decode_interval is the device lane's text - the block store after every scan), and over every
truncation of two files and 400 seeded corruptions of each: OK, INVALID or UNSUPPORTED comes back, never a sanitizer report."""
import json
import shutil
import subprocess
import zlib
from pathlib import Path

import pytest

import jpeg_prog_scenes
import ref_jpeg_prog

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/jpeg_prog_host.cpp")
    out = tmp_path_factory.mktemp("jpeg_prog_host") / "jpeg_prog_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "jpeg_prog_host.cpp")])
    return out


def _run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    return res.stdout.strip().splitlines()[-1]


def _crc(lut):
    return zlib.crc32(lut.astype("<u2").tobytes())


def _want(data):
    h = ref_jpeg_prog.parse(data)
    met = {}
    coef, _ = ref_jpeg_prog.entropy_decode(h, met)
    scans = []
    for scan in h["scans"]:
        scans.append({"comps": scan["comps"], "ss": scan["ss"], "se": scan["se"], "ah": scan["ah"], "al": scan["al"],
                      "restart": scan["restart"] or scan["mcus"], "mcus": scan["mcus"],
                      "dc_luts": [_crc(scan["dc"][c]["lut"]) for c in scan["comps"] if c in scan["dc"]],
                      "ac_lut": _crc(scan["ac"]["lut"]) if scan["ac"] else None,
                      "intervals": [list(where) for _, where in ref_jpeg_prog.intervals(h["data"], scan)]})
    return {"code": 0, "width": h["width"], "height": h["height"], "components": len(h["comps"]), "hmax": h["hmax"], "vmax": h["vmax"],
            "mcus_x": h["mcus_x"], "mcus_y": h["mcus_y"], "bpm": h["bpm"], "focal": h["focal_length_35mm"], "subsequences": sum(met["subsequences"]),
            "ac_refinement_scans": sum(1 for s in h["scans"] if s["ss"] > 0 and s["ah"]), "quant": [c["quant"] for c in h["comps"]], "scans": scans,
            "decode": 0, "coef": zlib.crc32(coef.astype("<i2").tobytes()),
            "met": [met["longest_eob_run"], int(met["zrl_in_refinement"]), int(met["new_at_se_in_refinement"]), int(met["corrections_in_eob_run"])]}


@pytest.mark.parametrize("name", jpeg_prog_scenes.names())
def test_walk_and_decode_are_the_restated_ones(exe, tmp_path, name):
    data = jpeg_prog_scenes.scene(name)
    (tmp_path / "in.jpg").write_bytes(data)
    got = json.loads(_run(exe, "parse", tmp_path / "in.jpg"))
    levels = [s.pop("level") for s in got["scans"]]
    assert got == _want(data)
    # the launch order: a refinement lies behind every earlier scan of its component whose band overlaps its own
    for k, b in enumerate(got["scans"]):
        for a, la in zip(got["scans"][:k], levels[:k]):
            if b["ah"] and set(a["comps"]) & set(b["comps"]) and a["ss"] <= b["se"] and b["ss"] <= a["se"]:
                assert levels[k] > la
        assert b["ah"] or levels[k] == 0


def test_refused_files(exe, tmp_path):
    """The files the walk refuses get the restatement's code from the walk; those only the entropy decode refuses walk."""
    for name, (data, code) in sorted(jpeg_prog_scenes.refused().items()):
        (tmp_path / "in.jpg").write_bytes(data)
        got = json.loads(_run(exe, "parse", tmp_path / "in.jpg"))
        try:
            ref_jpeg_prog.parse(data)
        except ref_jpeg_prog.JpegError as err:
            assert err.code == code and got["code"] == code, name
            continue
        assert got["code"] == code or (got["code"] == 0 and got["decode"] == code), name   # (the program's walk cuts the intervals too)


def test_refused_seams(exe, tmp_path):
    """The seam scenes broken at their seams: the walk takes the misnumbered RSTn when it cuts the intervals, the two cut scans walk
    and their entropy decode refuses them."""
    for name, (data, code) in sorted(jpeg_prog_scenes.refused_seams().items()):
        (tmp_path / "in.jpg").write_bytes(data)
        got = json.loads(_run(exe, "parse", tmp_path / "in.jpg"))
        ref_jpeg_prog.parse(data)
        if name == "misnumbered_rst_257":
            assert got["code"] == code and got["reason"] == "a misnumbered or surplus RSTn"
        else:
            assert got["code"] == 0 and got["decode"] == code, name


@pytest.mark.parametrize("name", ["q_17x9_420", "p_refine_grey_rst"])
def test_truncations_and_corruptions(exe, tmp_path, name):
    data = jpeg_prog_scenes.scene(name)
    (tmp_path / "in.jpg").write_bytes(data)
    ok, invalid, unsupported = (int(v) for v in _run(exe, "fuzz", tmp_path / "in.jpg", 7, 400).split())
    assert ok + invalid + unsupported == len(data) + 400
    assert invalid >= data.index(b"\xff\xda") - 1   # every cut in front of the first scan
    assert unsupported > 0                          # a cut behind a whole scan leaves an incomplete progression
    assert ok > 0


def test_refusals_are_the_recorded_ones(exe, tmp_path):
    """Code and reason of every refused scene, and a CRC over the code and reason of every truncation and corruption in order,
    are those the walk gave before the two decoders shared it (tests/golden/jpeg_walk_reasons.json): a file with several
    defects is still refused for the same one."""
    golden = json.loads((ROOT / "tests" / "golden" / "jpeg_walk_reasons.json").read_text())["progressive"]
    scenes = jpeg_prog_scenes.refused()
    assert sorted(scenes) == sorted(golden["refused"])
    for name, (data, _) in sorted(scenes.items()):
        (tmp_path / "in.jpg").write_bytes(data)
        got = json.loads(_run(exe, "parse", tmp_path / "in.jpg"))
        assert [got["code"], got.get("reason", "")] == golden["refused"][name], name
    for name, crc in sorted(golden["fuzz"].items()):
        (tmp_path / "in.jpg").write_bytes(jpeg_prog_scenes.scene(name))
        res = subprocess.run([str(exe), "fuzz", str(tmp_path / "in.jpg"), "7", "400"], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
        assert res.stdout.strip().splitlines()[-2] == "reasons %d" % crc, name
