"""cybervision_amd/csrc/tiff_encode_common.hpp as plain C++ on the CPU: tests/cpp/tiff_out_host.cpp, its own executable built
with AddressSanitizer and UBSan, against tests/ref_tiff_out.py - the refusals, the strip layout and the default rows per strip,
the size bounds, the header and IFD bytes of every (channels, strips, compression, predictor) class, and the routines the
kernels share with the host: the LZW walk (lzw_byte / lzw_finish / lzw_code_width) and the PackBits walk of a row."""
import itertools
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_tiff
import ref_tiff_out as R
import tiff_out_scenes as S

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tests/cpp/tiff_out_host.cpp")
    out = tmp_path_factory.mktemp("tiff_out_host") / "tiff_out_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(out), str(ROOT / "tests" / "cpp" / "tiff_out_host.cpp")])
    return out


def run(exe, *args):
    res = subprocess.run([str(exe), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout + res.stderr)[-4000:]


def plan(exe, tmp_path, w, h, c, compression, predictor, rps, first_count=0):
    run(exe, "plan", w, h, c, compression, predictor, rps, first_count, tmp_path / "plan.bin")
    out = (tmp_path / "plan.bin").read_bytes()
    refusal, = struct.unpack_from("<I", out)
    if refusal:
        assert len(out) == 4
        return {1: R.INVALID, 2: R.UNSUPPORTED}[refusal], None, None
    return R.OK, struct.unpack_from("<6I2Q", out, 4), out[4 + 24 + 16:]


def test_header_classes(exe, tmp_path):
    """Every (channels, one strip | several, compression, predictor) class: the bytes in front of the arrays or the strip."""
    for c, (h, rps), compression, predictor in itertools.product((1, 2, 3, 4), ((5, 0), (5, 2), (1, 1)), (R.NONE, R.LZW, R.PACKBITS), (1, 2)):
        if predictor == 2 and compression != R.LZW:
            continue
        w = 7
        row_bytes, rows, strips = R.check(w, h, c, compression, predictor, rps)
        want, data_at = R.header(w, h, c, compression, predictor, rows, strips, first_count=1234)
        code, numbers, got = plan(exe, tmp_path, w, h, c, compression, predictor, rps, 1234)
        assert code == R.OK and got == want, (c, h, rps, compression, predictor)
        assert numbers[:3] == (row_bytes, rows, strips) and numbers[5] == data_at
        assert numbers[3:5] == ((len(want), len(want) + 4 * strips) if strips > 1 else (0, 0))
        assert numbers[6] == R.worst_strip(compression, rows, row_bytes)


@pytest.mark.parametrize("name", S.names())
def test_scene_headers(exe, tmp_path, name):
    pixels, compression, predictor, rps = S.scene(name)
    data, stats, sections = S.expected(name)
    h, w, c = pixels.shape
    first = R.strips_of(data)[0][1]
    code, numbers, got = plan(exe, tmp_path, w, h, c, compression, predictor, rps, first)
    assert code == R.OK and numbers[2] == stats["strips"] and numbers[5] == sections[0]
    assert got == data[:len(got)] and len(got) == (sections[0] if stats["strips"] == 1 else numbers[3])
    if compression == R.NONE:
        assert numbers[7] == len(data)
    assert all(n <= numbers[6] for _, n in R.strips_of(data))   # the scratch stride holds every strip


def test_default_rows_per_strip_and_bounds(exe, tmp_path):
    for w, c in ((1, 1), (33, 1), (2047, 4), (2048, 4), (2049, 4), (8192, 1), (8191, 1), (8193, 1), (65535, 4), (4097, 1), (4096, 1), (2731, 3)):
        code, numbers, _ = plan(exe, tmp_path, w, 65535, c, R.LZW, 2, 0)
        assert code == R.OK and numbers[1] == R.default_rows_per_strip(w * c) == max(1, 8192 // (w * c)), (w, c)
    # rows_per_strip above the height is clamped; a strip just below 2^31 bytes is taken, at it refused
    assert plan(exe, tmp_path, 5, 7, 1, R.NONE, 1, 4000000000)[1][1:3] == (7, 1)
    assert plan(exe, tmp_path, 65535, 65535, 1, R.LZW, 1, 32768)[0] == R.OK   # 2^31 - 32768 bytes
    assert plan(exe, tmp_path, 65535, 65535, 1, R.LZW, 1, 32769)[0] == R.UNSUPPORTED
    assert plan(exe, tmp_path, 32768, 65535, 1, R.LZW, 1, 65535)[0] == R.OK   # 2^31 - 32768
    assert plan(exe, tmp_path, 32768, 65535, 2, R.LZW, 1, 32768)[0] == R.UNSUPPORTED   # 2^31
    # an uncompressed file's size is known up front: 2^32 - 1 is taken, 2^32 refused (65535 x 65535 x 1, one row a strip, is past it)
    code, numbers, _ = plan(exe, tmp_path, 65535, 65535, 1, R.NONE, 1, 16384)
    assert code == R.OK and numbers[7] < 2 ** 32
    for args in ((65535, 65535, 1, R.NONE, 1, 16384), (65535, 65535, 1, R.NONE, 1, 1), (32768, 65535, 2, R.NONE, 1, 2), (65535, 32768, 2, R.NONE, 1, 4)):
        want = R.OK
        try:
            R.check(*args)
        except R.TiffOutError as e:
            want = e.code
        assert plan(exe, tmp_path, *args)[0] == want, args
    assert plan(exe, tmp_path, 65535, 65535, 1, R.NONE, 1, 1)[0] == R.UNSUPPORTED


@pytest.mark.parametrize("name", sorted(S.REFUSED))
def test_refusals(exe, tmp_path, name):
    args, code = S.REFUSED[name]
    assert plan(exe, tmp_path, *args)[0] == code


def test_code_widths(exe, tmp_path):
    run(exe, "widths", tmp_path / "w.bin")
    assert list((tmp_path / "w.bin").read_bytes()) == [ref_tiff.code_width(c) for c in range(4096)]


def lzw_inputs():
    out = [(n, S.scene(n)[0].tobytes()) for n in ("lzw_last_code_3835", "lzw_last_code_3836", "lzw_last_code_3837", "lzw_flat", "lzw_1x1",
                                                 "lzw_width_254", "lzw_width_766", "lzw_width_1790", "lzw_noise_8192_one_strip", "lzw_strip_64k")]
    # the kernel's staging seams (the walk is shared): the densest stagings, a table-full Clear at each end of one, strings longer
    # than a staging, a strip close to its bound
    out += [(n, S.strip_bytes(n)[0]) for n in ("lzw_dense_4096", "lzw_clear_at_1022", "lzw_clear_at_1023", "lzw_clear_at_0", "lzw_clear_at_1",
                                                "lzw_dense_strips", "lzw_flat_640k")]
    out.append(("noise_40000", S.noise(40000, 41).tobytes()))
    out.append(("two_letters", np.random.default_rng(42).integers(0, 2, size=30000, dtype=np.uint8).tobytes()))
    return out


@pytest.mark.parametrize("name,data", lzw_inputs(), ids=[n for n, _ in lzw_inputs()])
def test_lzw_walk(exe, tmp_path, name, data):
    (tmp_path / "in.bin").write_bytes(data)
    run(exe, "lzw", tmp_path / "in.bin", tmp_path / "out.bin")
    out = (tmp_path / "out.bin").read_bytes()
    codes = R.lzw_codes(data)
    assert out[:-8] == R.lzw_pack(codes)
    assert struct.unpack("<2I", out[-8:]) == (len(codes), codes.count(R.CLEAR))
    assert len(out) - 8 <= R.worst_strip(R.LZW, 1, len(data))


def test_packbits_rows(exe, tmp_path):
    rng = np.random.default_rng(43)
    cases = [S.scene(n)[0].reshape(S.scene(n)[0].shape[0], -1) for n in S.names() if S.scene(n)[1] == R.PACKBITS]
    cases += [rng.integers(0, 2, size=(400, w), dtype=np.uint8) for w in (1, 2, 3, 4, 7, 127, 128, 129, 130, 131, 258, 300)]
    cases.append(np.stack([np.arange(1000) % 251] * 2).astype(np.uint8))   # all literal: the bound is met
    for rows in cases:
        rows.tofile(tmp_path / "in.bin")
        run(exe, "packbits", rows.shape[1], tmp_path / "in.bin", tmp_path / "out.bin")
        out, at = (tmp_path / "out.bin").read_bytes(), 0
        for row in rows:
            row = row.tobytes()
            walk = R.packbits_row(row)
            want = R.packbits_bytes(row, walk)
            size, packets = struct.unpack_from("<2I", out, at)
            assert (size, packets) == (len(want), len(walk)) and out[at + 8:at + 8 + size] == want
            assert size <= R.worst_strip(R.PACKBITS, 1, len(row))
            at += 8 + size
        assert at == len(out)
