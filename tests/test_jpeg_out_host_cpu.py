"""cybervision_amd/csrc/jpeg_encode_common.hpp as plain C++ on the CPU: tests/cpp/jpeg_out_host.cpp, its own executable built
with AddressSanitizer and UBSan, against tests/ref_jpeg_out.py - the quality scaling, the optimal tables from a histogram, the
code table the kernels read, the geometry and the segments in front of the scan."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_out_scenes
import ref_jpeg_out

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/jpeg_out_host.cpp")
    out = tmp_path_factory.mktemp("jpeg_out_host") / "jpeg_out_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "jpeg_out_host.cpp")])
    return out


def run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]


def test_quality_scaling(exe, tmp_path):
    run(exe, "quant", tmp_path / "q.bin")
    got = np.fromfile(tmp_path / "q.bin", dtype="<u2").reshape(100, 2, 64)
    for q in range(1, 101):
        assert (got[q - 1, 0] == ref_jpeg_out.quant_table(ref_jpeg_out.QUANT_LUMA, q)).all(), q
        assert (got[q - 1, 1] == ref_jpeg_out.quant_table(ref_jpeg_out.QUANT_CHROMA, q)).all(), q
    assert got.min() == 1 and got.max() == 255


def histograms():
    rng = np.random.RandomState(31)
    out = [("%s_%d" % (name, k), h) for name in sorted(jpeg_out_scenes.scenes())
           for k, h in enumerate(jpeg_out_scenes.restated(name)["histograms"])]
    one, two = [0] * 256, [0] * 256
    one[7] = 9
    two[0], two[255] = 4, 4
    out += [("one_symbol", one), ("two_symbols", two), ("all_equal", [3] * 256), ("none", [0] * 256)]
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    out.append(("fibonacci", [0] * 100 + fib + [0] * 116))
    out.append(("fibonacci_and_many", [1] * 100 + fib + [2] * 116))
    out.append(("powers_of_two", [0] * 30 + [1 << k for k in range(40)] + [0] * 186))
    big = [0] * 256
    big[0], big[3], big[200], big[255] = (1 << 32) + 5, 1 << 33, 1, (1 << 40) + 1
    out.append(("past_32_bits", big))
    for k in range(6):
        h = rng.randint(0, 1000, size=256) * (rng.rand(256) < (0.1 + 0.15 * k))
        out.append(("random_%d" % k, [int(v) for v in h]))
    return out


def test_optimal_tables_and_codes(exe, tmp_path):
    cases = histograms()
    np.array([h for _n, h in cases], dtype=np.uint64).tofile(tmp_path / "hist.bin")
    run(exe, "tables", tmp_path / "hist.bin", tmp_path / "out.bin")
    out, at = (tmp_path / "out.bin").read_bytes(), 0
    for name, hist in cases:
        bits, values = ref_jpeg_out.optimal_table(hist)
        unfolded = max(max(ref_jpeg_out.optimal_lengths_unfolded(hist)), 16)
        longest, = struct.unpack("<I", out[at:at + 4])
        total, = struct.unpack("<I", out[at + 20:at + 24])
        assert longest == unfolded, name
        assert list(out[at + 4:at + 20]) == bits, name
        assert total == len(values) == sum(bits) and list(out[at + 24:at + 24 + total]) == values, name
        codes = ref_jpeg_out.code_table(bits, values)
        want = [codes[s][1] << 16 | codes[s][0] if s in codes else 0 for s in range(256)]
        assert list(struct.unpack("<256I", out[at + 280:at + 280 + 1024])) == want, name
        at += 280 + 1024
        # a prefix code that keeps the all-ones code free: Kraft's sum stays below 1
        assert sum(n << (16 - k - 1) for k, n in enumerate(bits)) < 1 << 16 or not any(hist), name
        if name.startswith("fibonacci") or name == "powers_of_two":
            assert unfolded > 16 and max(k + 1 for k, n in enumerate(bits) if n) == 16, name
    assert at == len(out)
    # a chain deeper than the 32 at which libjpeg itself gives up: the fold here starts from any depth
    assert max(ref_jpeg_out.optimal_lengths_unfolded(dict(cases)["powers_of_two"])) > 32


def test_kernel_table_of_the_annex_k_tables(exe, tmp_path):
    run(exe, "kernel_table", tmp_path / "t.bin")
    got = np.fromfile(tmp_path / "t.bin", dtype="<u4")
    want = []
    for pair in range(2):
        dc = ref_jpeg_out.code_table(*ref_jpeg_out.STANDARD_TABLES[2 * pair])
        ac = ref_jpeg_out.code_table(*ref_jpeg_out.STANDARD_TABLES[2 * pair + 1])
        want += [dc[s][1] << 16 | dc[s][0] if s in dc else 0 for s in range(16)]
        want += [ac[s][1] << 16 | ac[s][0] if s in ac else 0 for s in range(256)]
    assert list(got) == want


@pytest.mark.parametrize("name", sorted(jpeg_out_scenes.scenes()))
def test_header_and_geometry(exe, tmp_path, name):
    pixels, quality, sampling, optimize = jpeg_out_scenes.scenes()[name]
    want = jpeg_out_scenes.restated(name)
    h, w = pixels.shape[:2]
    c = 1 if pixels.ndim == 2 else pixels.shape[2]
    hist = "-"
    if optimize:
        hist = tmp_path / "hist.bin"
        np.array(want["histograms"], dtype=np.uint64).tofile(hist)
    run(exe, "header", w, h, c, quality, sampling, hist, tmp_path / "out.bin")
    out = (tmp_path / "out.bin").read_bytes()
    n = want["sections"][0]
    assert out[:n] == want["file"][:n] and len(out) == n + 11 * 4 + 16
    g = ref_jpeg_out.geometry(w, h, 1 if c <= 2 else 3, sampling)
    geo = struct.unpack("<11I", out[n:n + 44])
    assert geo == (w, h, c, 1 if c <= 2 else 3, g["hs"], g["vs"], g["mcus_x"], g["mcus_y"], g["blocks_x"], g["blocks_y"], g["blocks_per_mcu"])
    assert struct.unpack("<2Q", out[n + 44:]) == (want["stats"]["blocks"], want["stats"]["dummy_blocks"])
