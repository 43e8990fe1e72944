"""cybervision_amd/csrc/png_common.hpp as plain C++ on the CPU: tests/cpp/png_host.cpp, its own executable built with
AddressSanitizer and UBSan, against tests/ref_png.py (code lengths, header bits, the token table) and against zlib (the
CRC-32 and Adler-32 of a buffer combined from its pieces)."""
import shutil
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import png_scenes
import ref_png

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/png_host.cpp")
    out = tmp_path_factory.mktemp("png_host") / "png_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "png_host.cpp")])
    return out


def histograms():
    rng = np.random.RandomState(21)
    out = [(name, png_scenes.restated(name)["histogram"]) for name in sorted(png_scenes.scenes())]
    lone = [0] * 286
    lone[9], lone[256] = 5, 1
    out.append(("two_symbols", lone))
    out.append(("all_equal", [3] * 286))
    out.append(("powers", [1 << min(s, 40) for s in range(286)]))
    for k in range(6):
        h = rng.randint(0, 1000, size=286) * (rng.rand(286) < (0.1 + 0.15 * k))
        h[256] = 1
        out.append(("random_%d" % k, [int(v) for v in h]))
    big = [0] * 286
    big[0], big[255], big[256], big[285] = (1 << 32) - 3, 1 << 31, 1, 7
    out.append(("past_32_bits", big))
    return out


def want_table(lengths):
    codes = ref_png.canonical_codes(lengths)
    table = []
    for t in range(513):
        extra = value = 0
        if t < 256:
            s = t
        elif t == 512:
            s = 256
        else:
            s, extra, value = ref_png.length_symbol(t - 256 + 3)
        n = lengths[s]
        if not n:
            table.append(0)
            continue
        bits = int(format(codes[s], "0%db" % n)[::-1], 2)
        if 256 <= t < 512:
            bits |= value << n
            n += extra + 1
        table.append(bits | n << 24)
    return table


def test_codes_and_header(exe, tmp_path):
    cases = histograms()
    np.array([h for _n, h in cases], dtype=np.uint64).tofile(tmp_path / "hist.bin")
    res = subprocess.run([str(exe), "codes", str(tmp_path / "hist.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
    out, at = (tmp_path / "out.bin").read_bytes(), 0
    for name, hist in cases:
        lengths = ref_png.package_merge(hist, 15)
        writer, parts = ref_png.block_header(lengths)
        assert list(out[at:at + 286]) == lengths, name
        assert list(out[at + 286:at + 305]) == parts["cl_lengths"], name
        hlit, hclen, nbits, nbytes = struct.unpack("<4I", out[at + 305:at + 321])
        at += 321
        assert (hlit, hclen, nbits) == (parts["hlit"], parts["hclen"], writer.n), name
        assert out[at:at + nbytes] == writer.tobytes(), name
        at += nbytes
        assert list(struct.unpack("<513I", out[at:at + 4 * 513])) == want_table(lengths), name
        at += 4 * 513
    assert at == len(out)


def test_checksums_combine(exe, tmp_path):
    rng = np.random.RandomState(22)
    for size in (0, 1, 7, 70_001, 300_000):
        buf = rng.randint(0, 256, size=size).astype(np.uint8)
        if size == 300_000:
            buf[:] = 0xFF  # the largest sums
        buf.tofile(tmp_path / "buf.bin")
        lines = ["", "0", str(size), "0 0 %d %d" % (size, size)]
        for _ in range(12):
            lines.append(" ".join(str(v) for v in sorted(rng.randint(0, size + 1, size=rng.randint(1, 9)))))
        (tmp_path / "splits.txt").write_text("\n".join(lines) + "\n")
        res = subprocess.run([str(exe), "sums", str(tmp_path / "buf.bin"), str(tmp_path / "splits.txt")], capture_output=True, text=True,
                             timeout=300)
        assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]
        got = [tuple(int(v) for v in line.split()) for line in res.stdout.splitlines()]
        assert got == [(zlib.crc32(buf.tobytes()), zlib.adler32(buf.tobytes()))] * len(lines), size
