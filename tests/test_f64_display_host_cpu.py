"""cybervision_amd/csrc/f64_display.hpp as plain C++ on the CPU: tests/cpp/f64_display_host.cpp, its own executable built with
AddressSanitizer and UBSan, against tests/ref_obj.py on the whole value set (obj_scenes.value_set: ~1.23 M doubles).  The
program itself cross-checks its digits against std::to_chars and its integer pair against std::to_string."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import obj_scenes
import ref_obj

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/f64_display_host.cpp")
    out = tmp_path_factory.mktemp("f64_display_host") / "f64_display_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "f64_display_host.cpp")])
    return out


def test_value_set(exe, tmp_path):
    values = obj_scenes.value_set()
    assert len(values) > 1_200_000
    values.tofile(tmp_path / "values.bin")
    res = subprocess.run([str(exe), str(tmp_path / "values.bin"), str(tmp_path / "strings.txt"), str(tmp_path / "lengths.bin")],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    assert json.loads(res.stdout.strip().splitlines()[-1]) == {"values": len(values), "bad": 0}
    got = (tmp_path / "strings.txt").read_bytes().split(b"\n")
    lengths = np.fromfile(tmp_path / "lengths.bin", dtype=np.uint32)
    assert got[-1] == b"" and len(got) == len(values) + 1 and len(lengths) == len(values)
    want = [ref_obj.display_a(v).encode("ascii") for v in values.tolist()]
    wrong = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not wrong, [(values[i].hex(), got[i], want[i]) for i in wrong[:5]]
    assert (lengths == np.fromiter((len(w) for w in want), dtype=np.uint32, count=len(want))).all()


def test_power_table_is_the_generators():
    """The committed f64_pow10.inc is what scripts/gen_f64_pow10.py writes (which also checks the header's fixed-point logarithms)."""
    assert subprocess.run([sys.executable, str(ROOT / "scripts" / "gen_f64_pow10.py"), "--check"]).returncode == 0
