"""Pyramid levels: SourceImage::resize = the `image` crate's Lanczos3
(reconstruction.rs:146-162).  The crate is not vendored with the reference, so nothing pins either side to it
("parity unpinned"); but the device (weights from glibc sinf on the host, f32 accumulation in tap order, no
contraction) and the oracle's numpy restatement (the same glibc sinf through ctypes, the same single IEEE f32
operations in the same order) must agree BIT FOR BIT: byte output, MAX_DIFF = 0.  The oracle itself is pinned to libm's
sinf and to an independent float64 statement of the formula (ref_resize.py), and mutants of it show which images can see
a fused accumulation, another sine, a reciprocal, another tap order or another rounding."""
import ctypes
import functools

import numpy as np
import pytest

import ref_resize
from cybervision_amd import synth

MAX_DIFF = 0            # grey levels: byte output is bit-exact against the oracle
MAX_FRACTION = 0.0      # of the pixels


@pytest.fixture(scope="module")
def lz():
    from oracle import cvref_resize

    return cvref_resize


def test_lanczos3_known_answers(lz):
    """Weights are normalised per output sample: a constant image stays constant; equal dimensions are a copy; the
    kernel is the Lanczos window (1 at 0, 0 at the other integers and beyond +-3); downsampling a smooth ramp by 2
    reproduces the ramp sampled at the new pixel centres; dims follow (w as f32 * scale) as u32."""
    c = np.full((90, 130), 201, dtype=np.uint8)
    assert (lz.resize_lanczos3(c, 41, 33) == 201).all()
    a, _, _ = synth.make_pair(96, 80, seed=5)
    assert (lz.resize_lanczos3(a, 96, 80) == a).all()
    k = lz.lanczos3_kernel(np.array([0.0, 1.0, 2.0, 3.0, 3.5, -1.0, 0.5], dtype=np.float32))
    assert k[0] == 1.0 and np.abs(k[1:3]).max() < 1e-6 and k[3] == 0.0 and k[4] == 0.0 and abs(k[5]) < 1e-6
    assert abs(k[6] - (np.sin(np.pi / 2) / (np.pi / 2)) * (np.sin(np.pi / 6) / (np.pi / 6))) < 1e-6
    ramp = np.tile(np.arange(40, 200, dtype=np.uint8)[None, :], (64, 1))
    half = lz.resize_lanczos3(ramp, 80, 32)
    want = 40 + 2 * np.arange(80) + 0.5
    assert np.abs(half[16, 4:-4] - want[4:-4]).max() <= 1.0
    assert lz.resize_scale(np.zeros((75, 101), dtype=np.uint8), 0.25).shape == (18, 25)
    # overshoot is clamped, not wrapped: a hard edge stays within [0, 255]
    edge = np.zeros((64, 64), dtype=np.uint8)
    edge[:, 32:] = 255
    out = lz.resize_lanczos3(edge, 32, 32)
    assert out.min() == 0 and out.max() == 255


@pytest.mark.gpu
@pytest.mark.parametrize("dims,scale", [((512, 384), 0.5), ((1000, 700), 0.25), ((333, 517), 0.125), ((256, 256), 1.0),
                                        ((2048, 2048), 1.0 / 32)])
def test_device_lanczos3_matches_numpy_restatement(gpu_device, lz, dims, scale):
    from cybervision_amd import correlation

    a, _, _ = synth.make_pair(dims[0], dims[1], seed=dims[0] % 97, sem_style=True)
    want = lz.resize_scale(a, scale)
    got = correlation.resize_lanczos3(gpu_device, a, scale)
    assert got.shape == want.shape and got.dtype == np.uint8
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= MAX_DIFF, d.max()
    assert (d > 0).mean() <= MAX_FRACTION, (d > 0).mean()


@pytest.mark.gpu
def test_device_lanczos_pyramid_resident(gpu_device, lz):
    """The level loop's pyramid, built on the device from a device-resident image and kept there."""
    import torch

    from cybervision_amd import correlation

    a, _, _ = synth.make_pair(640, 480, seed=3)
    pyr = correlation.lanczos_pyramid(gpu_device, torch.from_numpy(a).cuda(), 2)
    assert [tuple(p.shape) for p in pyr] == [(480, 640), (240, 320), (120, 160)] and all(p.is_cuda for p in pyr)
    assert (pyr[0].cpu().numpy() == a).all()
    for k in (1, 2):
        d = np.abs(pyr[k].cpu().numpy().astype(np.int32) - lz.resize_scale(a, 1.0 / (1 << k)).astype(np.int32))
        assert d.max() <= MAX_DIFF and (d > 0).mean() <= MAX_FRACTION


# ---------------------------------------------------------------------------------------------------------------------
# The oracle against libm and against an independent float64 reference, and the device against both, at the shapes where
# the entry point takes another path.  Everything below goes through the C entry point with (w, h) -> (nw, nh).
# ---------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def _image(w, h, seed):
    """Values from {0, 255} only in the left half of the columns, noise in the right half.  (The f32 centre of a tap window
    is the less exact the further right it lies, and the hard half has the steeper gradients: this way round the f32
    oracle stays near enough to the f64 reference for MAX_EXCLUDED at every shape below.)"""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    hard = (rng.integers(0, 2, size=(h, w), dtype=np.uint8) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.where(np.arange(w)[None, :] < w // 2, hard, noise))


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


# (w, h), (nw, nh), seed of _image, delta.  delta = twice the largest |oracle's unrounded f32 value - f64 value| of the case,
# rounded up; the measured largest difference is in the comment (it is the rounding of the f32 tap centre and window
# argument times the image's gradient, not the accumulation's error: it grows with the source coordinate).
SHAPE_CASES = [
    ((37, 29), (37, 13), 1, 3.6e-4),        # 1.79e-4; one axis kept
    ((40, 30), (41, 30), 1, 1.2e-3),        # 5.50e-4; one axis kept, the other upsampled
    ((64, 48), (100, 75), 1, 2.8e-3),       # 1.39e-3; upsampling (0.41 % of the pixels within delta of k + 1/2)
    ((2, 2), (3, 3), 1, 6.1e-5),            # 3.0e-5; tiny upsample
    ((1, 1), (5, 7), 2, 1e-6),              # 0; 1 x 1 source (every weight row is the single 1.0)
    ((64, 48), (1, 1), 1, 2e-6),            # 9.9e-7; 1 x 1 output
    ((6, 6), (1, 6), 1, 1.8e-5),            # 8.55e-6; output 1 pixel wide
    ((300, 7), (7, 300), 1, 4.4e-4),        # 2.17e-4; opposite ratios on the two axes
    ((5, 5), (4, 4), 1, 6.2e-5),            # 3.07e-5; small non-dyadic downscale
    ((2000, 8), (3, 8), 1, 6.9e-4),         # 3.41e-4; about 4000 taps per output
    ((257, 255), (128, 127), 2, 1.8e-3),    # 8.83e-4; sizes next to the 256-lane block (0.40 %)
    ((513, 100), (255, 50), 8, 4.1e-3),     # 2.01e-3; output widths across the 256-lane block edge (0.71 %)
    ((513, 100), (256, 50), 1, 1.9e-4),     # 9.15e-5
    ((513, 100), (257, 50), 12, 4.1e-3),    # 2.00e-3 (0.62 %)
]
# the images on which the mutants of test_oracle_mutants_change_bytes were searched: noise, about 1e6 output pixels
# at a ratio that is no halving, sources up to 2048.  The outputs are 1024 wide and high so that ratio = in / 1024 and the
# tap centres (2 o + 1) in / 2048 are exact in f32: with rounded centres (1536 -> 1000) the f32 restatement is 0.015 grey
# levels from the f64 reference, 5.9 % of the pixels lie within twice that of k + 1/2, and MAX_EXCLUDED cannot hold.  Such a
# pair is compared with the oracle alone (test_device_inexact_centres_at_full_size).
SENSITIVE_CASES = [
    ((1800, 2000), (1024, 1024), 1, 2.2e-4),    # 1.08e-4 (0.04 %)
    ((1416, 1800), (1024, 1024), 3, 2.1e-4),    # 1.03e-4 (0.05 %)
    ((1600, 2040), (1024, 1024), 2, 2.1e-4),    # 1.04e-4 (0.04 %)
]
# bytes changed by each mutant on these three images, in their order, where the seeds were searched (glibc 2.x, numpy 2.2
# with its AVX-512 sine): fused 5 + 9 + 8, numpy's sine 8 + 7 + 6, reciprocal 11 + 10 + 8, reverse order 14 + 11 + 13, half
# to even 7 + 4 + 5
HARD_CONTRAST = ((64, 48), (100, 75))
MAX_EXCLUDED = 0.01     # of a case's pixels may lie within delta of k + 1/2


def _case_id(c):
    return "%dx%d-%dx%d" % (c[0] + c[1])


@functools.lru_cache(maxsize=None)
def _case(dims, new, seed, sensitive=False):
    """(image, oracle's unclamped f32, oracle's bytes, f64 values) of one case, computed once; read-only."""
    from oracle import cvref_resize as lz

    img = _noise(dims[0], dims[1], seed) if sensitive else _image(dims[0], dims[1], seed)
    f32 = lz.resample_f32(img, new[0], new[1])
    out = (img, f32, lz.to_u8(f32), ref_resize.resample_f64(img, new[0], new[1]))
    for a in out:
        a.setflags(write=False)
    return out


def _assert_matches_f64(got, v64, delta):
    """Bytes equal the f64 reference's, except within delta of k + 1/2 where they may differ by one; few such pixels."""
    want = ref_resize.to_u8(v64)
    v = np.clip(v64, 0.0, 255.0)
    near = np.abs(v - np.floor(v) - 0.5) <= delta
    assert near.mean() <= MAX_EXCLUDED, near.mean()
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert (d[~near] == 0).all(), (int((d[~near] != 0).sum()), int(d.max()))
    assert d.max() <= 1, d.max()


def _libm_sinf():
    libm = ctypes.CDLL("libm.so.6")
    libm.sinf.restype, libm.sinf.argtypes = ctypes.c_float, [ctypes.c_float]
    return libm.sinf


def _sine_arguments(lz, in_size, out_size):
    """Every argument the taps of (in_size, out_size) give to the sine: pi x and pi (x / 3), f32, formed as the oracle does."""
    ratio = F32(in_size) / F32(out_size)
    sratio = F32(1.0) if ratio < F32(1.0) else ratio
    args = []
    for o in range(out_size):
        centre = (F32(o) + F32(0.5)) * ratio
        left = min(max(int(np.floor(centre - F32(3.0) * sratio)), 0), in_size - 1)
        right = min(max(int(np.ceil(centre + F32(3.0) * sratio)), left + 1), in_size)
        x = (np.arange(left, right).astype(F32) - (centre - F32(0.5))) / sratio
        x = x[np.abs(x) < F32(3.0)]
        args += [x * F32(np.pi), (x / F32(3.0)) * F32(np.pi)]
    return np.concatenate(args).astype(F32)


def test_oracle_sine_is_libm_sinf(lz):
    """The oracle's sine is the running machine's libm sinf, bit for bit: on every argument the taps of two non-dyadic size
    pairs produce, and on 4096 arguments spread over the kernel's range (|x| < 3: |pi x| < 3 pi)."""
    sinf = _libm_sinf()
    args = np.concatenate([_sine_arguments(lz, 1536, 1000), _sine_arguments(lz, 601, 900),
                           np.random.default_rng(1).uniform(-3 * np.pi, 3 * np.pi, 4096).astype(F32)])
    assert args.size > 8000
    want = np.array([sinf(float(v)) for v in args], dtype=F32)
    got = lz.sinf(args)
    assert got.dtype == F32 and (got.view(np.uint32) == want.view(np.uint32)).all()
    # and it is what the window is made of: sinc(x) = sinf(pi x) / (pi x), one f32 operation each
    x = args[:2000][args[:2000] != 0] / F32(np.pi)
    a = x * F32(np.pi)
    assert (lz._sinc(x).view(np.uint32) == (np.array([sinf(float(v)) for v in a], dtype=F32) / a).view(np.uint32)).all()


@pytest.mark.parametrize("case", SHAPE_CASES + [c + (True,) for c in SENSITIVE_CASES], ids=_case_id)
def test_oracle_matches_f64_reference(lz, case):
    """The f32 restatement against the matrix form in float64: no NaN, no zero weight sum, the unrounded values within
    delta / 2, the bytes equal except within delta of k + 1/2."""
    dims, new, seed, delta = case[:4]
    img, f32, out, v64 = _case(dims, new, seed, len(case) > 4)
    assert np.isfinite(f32).all() and np.isfinite(v64).all()
    for n_in, n_out in ((dims[1], new[1]), (dims[0], new[0])):
        for o in range(0, n_out, max(1, n_out // 64)):
            assert np.isfinite(lz.taps_of(n_in, n_out)[o][1]).all()
    err = np.abs(f32.astype(np.float64) - v64).max()
    print("%s: largest |f32 - f64| = %.3g, delta = %.3g" % (_case_id(case), err, delta))
    assert 2 * err <= delta, (err, delta)
    _assert_matches_f64(out, v64, delta)


# ---- mutants: each differs from the oracle in ONE rule that the device could get wrong --------------------------------
def _mutant_axis0(lz, img_f32, out_size, tables, fused, recip, reverse):
    h, w = img_f32.shape
    out = np.zeros((out_size, w), dtype=F32)
    key = (h, out_size)
    if key not in tables:
        tables[key] = [lz._raw_taps(h, out_size, o) for o in range(out_size)]
    for o, (left, raw) in enumerate(tables[key]):
        total = F32(0.0)
        for v in raw:
            total = F32(total + v)
        ws = (raw * (F32(1.0) / total)).astype(F32) if recip else (raw / total).astype(F32)
        t = np.zeros(w, dtype=F32)
        for i in (range(len(ws) - 1, -1, -1) if reverse else range(len(ws))):
            if fused:   # fl32(t + a b): a and b hold 24 bits each, so the f64 product is exact
                t = (t.astype(np.float64) + img_f32[left + i].astype(np.float64) * np.float64(ws[i])).astype(F32)
            else:
                t = (t + img_f32[left + i] * ws[i]).astype(F32)
        out[o] = t
    return out


def _mutant(lz, img, nw, nh, tables, fused=False, recip=False, reverse=False, half_even=False):
    tmp = _mutant_axis0(lz, img.astype(F32), nh, tables, fused, recip, reverse)
    out = _mutant_axis0(lz, np.ascontiguousarray(tmp.T), nw, tables, fused, recip, reverse).T
    if half_even:
        return np.rint(np.clip(out, F32(0.0), F32(255.0))).astype(np.uint8)
    return lz.to_u8(out)


def _numpy_sin(a):
    return np.sin(np.asarray(a, dtype=F32), dtype=F32)


def _mutant_counts(lz, monkeypatch, cases):
    """Bytes changed over `cases` by each mutant; (b) is None where numpy's f32 sine is libm's on this machine."""
    counts = {"fused": 0, "recip": 0, "reverse": 0, "half_even": 0, "numpy_sin": 0}
    probe = _sine_arguments(lz, 1536, 1000)
    same_sine = (_numpy_sin(probe).view(np.uint32) == lz.sinf(probe).view(np.uint32)).all()
    for dims, new, seed, _ in cases:
        img, _, want, _ = _case(dims, new, seed, True)
        tables = {}
        assert (_mutant(lz, img, new[0], new[1], tables) == want).all()      # the unmutated form is the oracle
        for k in ("fused", "recip", "reverse", "half_even"):
            counts[k] += int((_mutant(lz, img, new[0], new[1], tables, **{k: True}) != want).sum())
        if not same_sine:
            with monkeypatch.context() as m:
                m.setattr(lz, "sinf", _numpy_sin)
                counts["numpy_sin"] += int((_mutant(lz, img, new[0], new[1], {}) != want).sum())
    if same_sine:
        counts["numpy_sin"] = None
    return counts


def test_oracle_mutants_change_bytes(lz, monkeypatch):
    """Teeth: over the sensitive images, each of (a) fused accumulation in both passes, (b) numpy's own f32 sine, (c)
    weights times 1 / sum, (d) reverse tap order, (e) round half to even changes at least 2 bytes - so a device that gets one
    of these rules wrong cannot pass test_device_sensitive_images.
    The counts of the committed seeds are next to SENSITIVE_CASES."""
    counts = _mutant_counts(lz, monkeypatch, SENSITIVE_CASES)
    print("bytes changed by each mutant:", counts)
    for k, n in counts.items():
        assert n is None or n >= 2, counts


def test_oracle_overshoots_both_sides_of_the_clamp():
    """The hard-contrast case drives the unclamped result below 0 and above 255: both sides of the clamp are used."""
    case = next(c for c in SHAPE_CASES if (c[0], c[1]) == HARD_CONTRAST)
    _, f32, out, _ = _case(*case[:3])
    assert f32.min() < -1.0 and f32.max() > 256.0, (f32.min(), f32.max())
    assert out.min() == 0 and out.max() == 255


# ---- the device ---------------------------------------------------------------------------------------------------------
CVHIP_OK, CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED = 0, -1, -3


def _resize(dev, src, dims, dst, new):
    """cvhip_resize_lanczos3 on numpy arrays (host memory) or torch CUDA tensors (device memory); the return code."""
    from cybervision_amd import _lib

    def ptr(a):
        return ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)

    return _lib.lib().cvhip_resize_lanczos3(dev.handle, ptr(src), dims[0], dims[1], ptr(dst), new[0], new[1])


def _device_bytes(dev, img, new):
    out = np.full((new[1], new[0]), 0xA5, dtype=np.uint8)
    assert _resize(dev, img, (img.shape[1], img.shape[0]), out, new) == CVHIP_OK
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPE_CASES, ids=_case_id)
def test_device_shapes_match_oracle_and_f64(gpu_device, case):
    """One axis kept, upsampling, 1-pixel sources and outputs, opposite ratios, thousands of taps, the 256-lane block edge:
    bytes equal the oracle's, and the f64 reference's except within delta of k + 1/2."""
    dims, new, seed, delta = case
    img, _, want, v64 = _case(dims, new, seed)
    got = _device_bytes(gpu_device, img, new)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= MAX_DIFF, (int(d.max()), int((d > 0).sum()))
    _assert_matches_f64(got, v64, delta)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SENSITIVE_CASES, ids=_case_id)
def test_device_sensitive_images(gpu_device, case):
    """The images on which every mutant of test_oracle_mutants_change_bytes changes bytes: a contracted multiply-add,
    another sine, a reciprocal, another tap order or another rounding on the device would show here."""
    dims, new, seed, delta = case
    img, _, want, v64 = _case(dims, new, seed, True)
    got = _device_bytes(gpu_device, img, new)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= MAX_DIFF, (int(d.max()), int((d > 0).sum()))
    _assert_matches_f64(got, v64, delta)


@pytest.mark.gpu
def test_device_inexact_centres_at_full_size(gpu_device, lz):
    """1536 x 1536 -> 1000 x 1000: unlike the sensitive images, the ratio and the tap centres round in f32 (ulp 1.2e-4 at
    1024 and above), so the f32 restatement is up to 0.015 grey levels from the f64 reference (measured; 5.9 % of the
    pixels within twice that of k + 1/2) and only the oracle is compared: by equality."""
    img = _noise(1536, 1536, 1)
    got = _device_bytes(gpu_device, img, (1000, 1000))
    assert (got == lz.resize_lanczos3(img, 1000, 1000)).all()


PLACEMENT_RESAMPLE = ((513, 100), (257, 50))


@pytest.mark.gpu
@pytest.mark.parametrize("src_on_device", [False, True], ids=["host_src", "device_src"])
@pytest.mark.parametrize("dst_on_device", [False, True], ids=["host_dst", "device_dst"])
def test_device_placements(gpu_device, src_on_device, dst_on_device):
    """Source and destination each in host or in device memory, for a resampling call and for the equal-size copy; a
    device -> device result is read after a synchronise of the handle only."""
    import torch

    case = next(c for c in SHAPE_CASES if (c[0], c[1]) == PLACEMENT_RESAMPLE)
    img, _, want, _ = _case(*case[:3])
    dims = case[0]
    for new, expect in ((case[1], want), (dims, img)):
        src = torch.from_numpy(img.copy()).cuda() if src_on_device else img.copy()
        if dst_on_device:
            dst = torch.full((new[1], new[0]), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()      # (the fill runs on torch's stream, the resize on the handle's)
        else:
            dst = np.full((new[1], new[0]), 0xA5, dtype=np.uint8)
        assert _resize(gpu_device, src, dims, dst, new) == CVHIP_OK
        if src_on_device and dst_on_device:
            gpu_device.synchronize()
        got = dst.cpu().numpy() if dst_on_device else dst
        assert (got == expect).all(), new


# (w, h) -> (nw, nh) in call order.  A call looks its vertical table (h, nh) up first, then its horizontal one (w, nw); the
# cache is a std::vector that grows at 1, 2, 4 and 8 entries (libstdc++ doubles).  Entries after each call, and what the
# call is there for:
TABLE_CALLS = [
    ((40, 40), (30, 30)),    # 1 entry: square -> square, both passes use the one table (40, 30)
    ((50, 40), (35, 30)),    # 2: vertical (40, 30) cached, horizontal (50, 35) new with the vector full at 1: it moves
    ((60, 50), (45, 35)),    # 3: vertical (50, 35) cached, horizontal (60, 45) new with the vector full at 2: it moves
    ((50, 50), (35, 35)),    # 3: all cached, square -> square on a table that another call's horizontal pass made
    ((96, 64), (64, 96)),    # 5: both new; the second moves the vector, full at 4 with the first one just pushed
    ((70, 96), (31, 64)),    # 6: vertical (96, 64) cached - the HORIZONTAL table of the call before
    ((45, 60), (80, 45)),    # 7: vertical (60, 45) cached, horizontal (45, 80) new (upsampling)
    ((60, 33), (45, 44)),    # 8: vertical (33, 44) new, horizontal (60, 45) cached
    ((21, 64), (20, 96)),    # 9: vertical (64, 96) cached, horizontal (21, 20) new with the vector full at 8: it moves
    ((64, 21), (96, 20)),    # 9: all cached, each table in the other role
    ((33, 70), (44, 31)),    # 9: all cached
    ((40, 50), (30, 35)),    # 9: the first two entries, after four moves
]


@pytest.mark.gpu
def test_device_table_cache_growth(lz):
    """The table cache grows while a call holds a pointer into it; every result equals the oracle, and the whole sequence
    again - now all from the cache - gives the same bytes."""
    from cybervision_amd import correlation

    assert len(set(TABLE_CALLS)) == len(TABLE_CALLS) >= 10
    images = [_image(w, h, 100 + k) for k, ((w, h), _) in enumerate(TABLE_CALLS)]
    want = [lz.resize_lanczos3(img, *new) for img, (_, new) in zip(images, TABLE_CALLS)]
    dev = correlation.create_gpu_context()
    try:
        first = [_device_bytes(dev, img, new) for img, (_, new) in zip(images, TABLE_CALLS)]
        again = [_device_bytes(dev, img, new) for img, (_, new) in zip(images, TABLE_CALLS)]
    finally:
        dev.close()
    for k, (a, b, w) in enumerate(zip(first, again, want)):
        assert (a == w).all(), (k, TABLE_CALLS[k])
        assert (b == w).all(), (k, TABLE_CALLS[k])


PLANE_CALLS = [((40, 30), (20, 15)), ((700, 500), (333, 401)), ((64, 48), (100, 75)), ((900, 700), (601, 467))]


@pytest.mark.gpu
def test_device_plane_regrowth_in_stream_order(lz):
    """Device -> device calls small, large, small, larger on a fresh handle with no synchronise between them: the shared
    f32 plane is replaced twice while earlier calls may still be queued.  One synchronise, then all four equal the oracle."""
    import torch

    from cybervision_amd import correlation

    images = [_image(w, h, 200 + k) for k, ((w, h), _) in enumerate(PLANE_CALLS)]
    want = [lz.resize_lanczos3(img, *new) for img, (_, new) in zip(images, PLANE_CALLS)]
    srcs = [torch.from_numpy(img).cuda() for img in images]
    dsts = [torch.full((new[1], new[0]), 0xA5, dtype=torch.uint8, device="cuda") for _, new in PLANE_CALLS]
    torch.cuda.synchronize()
    dev = correlation.create_gpu_context()
    try:
        for src, dst, (dims, new) in zip(srcs, dsts, PLANE_CALLS):
            assert _resize(dev, src, dims, dst, new) == CVHIP_OK
        dev.synchronize()
        got = [d.cpu().numpy() for d in dsts]
    finally:
        dev.close()
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g == w).all(), (k, PLANE_CALLS[k])


@pytest.mark.gpu
def test_device_error_returns_write_nothing(gpu_device, lz):
    """Null pointers and empty images are CVHIP_ERR_INVALID, a dimension of 65 536 is CVHIP_ERR_UNSUPPORTED; the destination
    keeps its sentinel; the handle resizes correctly afterwards."""
    from cybervision_amd import _lib, correlation

    fn = _lib.lib().cvhip_resize_lanczos3
    img = _image(16, 12, 7)
    dst = np.full((64, 64), 0xA5, dtype=np.uint8)
    ps, pd, h = ctypes.c_void_p(img.ctypes.data), ctypes.c_void_p(dst.ctypes.data), gpu_device.handle
    calls = [((None, ps, 16, 12, pd, 8, 6), CVHIP_ERR_INVALID), ((h, None, 16, 12, pd, 8, 6), CVHIP_ERR_INVALID),
             ((h, ps, 16, 12, None, 8, 6), CVHIP_ERR_INVALID),
             ((h, ps, 0, 12, pd, 8, 6), CVHIP_ERR_INVALID), ((h, ps, 16, 0, pd, 8, 6), CVHIP_ERR_INVALID),
             ((h, ps, 16, 12, pd, 0, 6), CVHIP_ERR_INVALID), ((h, ps, 16, 12, pd, 8, 0), CVHIP_ERR_INVALID),
             # (the size checks come before anything is read or written: the buffers are never touched)
             ((h, ps, 65536, 12, pd, 8, 6), CVHIP_ERR_UNSUPPORTED), ((h, ps, 16, 65536, pd, 8, 6), CVHIP_ERR_UNSUPPORTED),
             ((h, ps, 16, 12, pd, 65536, 6), CVHIP_ERR_UNSUPPORTED), ((h, ps, 16, 12, pd, 8, 65536), CVHIP_ERR_UNSUPPORTED)]
    for args, code in calls:
        assert fn(*args) == code, args[2:]
        assert (dst == 0xA5).all(), args[2:]
    # a scale at which the wrapper computes a zero size
    with pytest.raises(_lib.CvhipError) as err:
        correlation.resize_lanczos3(gpu_device, img, 1.0 / 32)
    assert err.value.code == CVHIP_ERR_INVALID
    assert (_device_bytes(gpu_device, img, (8, 6)) == lz.resize_lanczos3(img, 8, 6)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.25, float(np.float32(1.0) / np.float32(3.0))], ids=["quarter", "third"])
def test_wrapper_dims_follow_the_f32_product(gpu_device, lz, scale):
    """correlation.resize_lanczos3 sizes its output like SourceImage::resize: (w as f32 * scale) as u32."""
    from cybervision_amd import correlation

    img = _image(101, 75, 9)
    want = lz.resize_scale(img, scale)
    got = correlation.resize_lanczos3(gpu_device, img, scale)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert (got == want).all()
