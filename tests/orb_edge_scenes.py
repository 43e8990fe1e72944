"""Scenes for tests/test_orb_edges_ref.py and tests/test_orb_edges_gpu.py: images and descriptor sets that reach the
branches of the sparse front end (adjust_contrast, the Harris ranking, the orientation, the matcher's two kernels) which
synth.make_pair + add_blocks and white noise of range 0..255 never take.  Everything is numpy with fixed seeds; images are
[h, w] uint8, descriptor sets [n, 8] uint32.

  stretch_scene(span)   noise of range exactly `span`: adjust_contrast's f32 quotient, product and round (orb.rs:468-470)
  periodic_scene()      a repeated tile: thousands of EQUAL Harris responses, the cut at MAX_KEYPOINTS inside a group
  dim_scene(levels)     values 0..levels-1: FAST sees the stretched image, the moments the original (m00 = 0 -> NaN angle)
  ragged_scene(w, h)    sizes around the stages' borders, widths and pixel counts that are no multiple of four
  *_descriptors(...)    matcher inputs around the switch between its two kernels and the seams of the candidate splits"""
import numpy as np

STRETCH_SHAPE = (96, 128)
MUTANT_SPANS = (6, 34, 102, 130, 170, 200)   # coeff * v hits exact halves at the first five; f32 != f64 shows at 200
PERIODIC_TILE = 32
PERIODIC_SHAPE = (384, 512)
PERIODIC_CROP = (128, 160)
DIM_SHAPE = (160, 200)
# (w, h): the first eight yield (almost) nothing, the last three some keypoints
RAGGED_SIZES = [(7, 7), (8, 7), (31, 31), (46, 46), (47, 47), (33, 64), (300, 40), (40, 300), (64, 300), (203, 97), (97, 203)]
RAGGED_WITH_KEYPOINTS = [(64, 300), (203, 97), (97, 203)]
# (n1, n2): one pair, one query, one past the vector kernel's 256-query block and 512-candidate tile and exactly on them, one
# pair below the switch to the matrix-pipe kernel (n1 * n2 >= 2^22) and exactly on it, one padded candidate tile, one
# workgroup that is mostly padding rows
MATCH_SIZES = [(1, 1), (1, 700), (257, 513), (256, 512), (2047, 2048), (2048, 2048), (140_000, 30), (33, 130_000)]
MATCH_SIZES_MATRIX_PIPE = [(2048, 2048), (140_000, 30), (33, 130_000)]
MATCH_THRESHOLDS = (0, 48, 256)
VECTOR_KERNEL_THRESHOLD = 0x4000  # no smaller threshold is refused by the matrix-pipe form; no distance exceeds 256
CLIP_N1, CLIP_N2 = 65_536, 140_000
CLIP_TARGETS = (65_535, 65_536, 65_537, 131_071, 131_072, 139_999)
CLIP_COPIES = (65_540, 131_073, 70_000, 131_080, 139_000, None)  # the equal later copy of each target's descriptor
CLIP_DECOY = 3  # ... the last index has no later place: its queries get a copy one bit WORSE, early in the list


# seed 0 everywhere but at span 200: there the f32 and the f64 coefficient differ at two values only (100 and 180), and seed 12
# is the first whose image has a corner that can reach the final list and hangs on one of them
STRETCH_SEEDS = {200: 12}


def stretch_scene(span, seed=None):
    """96 x 128 noise, uniform in [lo, lo + span], both extremes present; lo drawn so that lo + span <= 255."""
    assert 1 <= span <= 255
    seed = STRETCH_SEEDS.get(span, 0) if seed is None else seed
    rng = np.random.default_rng(1000 * seed + span)
    lo = int(rng.integers(0, 256 - span))
    img = (lo + rng.integers(0, span + 1, size=STRETCH_SHAPE)).astype(np.uint8)
    img[0, 0], img[0, 1] = lo, lo + span
    return img


def periodic_scene():
    rng = np.random.default_rng(32)
    tile = rng.integers(0, 256, size=(PERIODIC_TILE, PERIODIC_TILE), dtype=np.uint8)
    return np.ascontiguousarray(np.tile(tile, (PERIODIC_SHAPE[0] // PERIODIC_TILE, PERIODIC_SHAPE[1] // PERIODIC_TILE)))


def periodic_crop():
    return np.ascontiguousarray(periodic_scene()[:PERIODIC_CROP[0], :PERIODIC_CROP[1]])


def dim_scene(levels):
    """levels = 2: sparse ones on zeros (the blurred original stays below 1); levels = 4: uniform 0..3."""
    rng = np.random.default_rng(40 + levels)
    if levels == 2:
        return (rng.random(DIM_SHAPE) < 0.12).astype(np.uint8)
    return rng.integers(0, levels, size=DIM_SHAPE, dtype=np.uint8)


def ragged_scene(w, h):
    """The top left w x h of the periodic scene under a few grey levels of noise: its keypoints resemble the periodic
    crop's, at small non-zero descriptor distances (the fixture's matches)."""
    rng = np.random.default_rng(7000 + 1000 * w + h)
    img = periodic_scene()[:h, :w].astype(np.int64) + rng.integers(-6, 7, size=(h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def flat_scene():
    return np.full((40, 56), 77, dtype=np.uint8)


def low_span_scene():
    return stretch_scene(6)


def rich_scene():
    """More than 1 000 keypoints: for `cap` below the count."""
    rng = np.random.default_rng(77)
    return rng.integers(0, 256, size=(200, 260), dtype=np.uint8)


def mixed_batch():
    """Dim, flat, periodic, low-span and 7 x 7 in one batch."""
    return [dim_scene(2), flat_scene(), periodic_crop(), low_span_scene(), ragged_scene(7, 7), dim_scene(4)]


# ---- matcher inputs -------------------------------------------------------------------------------------------------
def rand_desc(rng, n):
    return rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)


def flip_bits(desc, counts, rng):
    """desc with counts[i] DISTINCT bits of row i flipped (positions start + c * stride mod 256, stride odd)."""
    n = len(desc)
    counts = np.asarray(counts)
    c = np.arange(max(int(counts.max(initial=0)), 1))
    start = rng.integers(0, 256, size=(n, 1))
    stride = 2 * rng.integers(0, 128, size=(n, 1)) + 1
    pos = (start + c[None] * stride) % 256
    flip = np.zeros((n, 256), dtype=np.uint8)
    rows = np.broadcast_to(np.arange(n)[:, None], pos.shape)
    sel = c[None] < counts[:, None]
    flip[rows[sel], pos[sel]] = 1
    return desc ^ np.packbits(flip, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def coords(n1, n2):
    xy1 = np.stack([np.arange(n1), np.arange(n1) + 3], axis=1).astype(np.uint32)
    xy2 = np.stack([np.arange(n2), 2 * np.arange(n2)], axis=1).astype(np.uint32)
    return xy1, xy2


def planted_descriptors(n1, n2):
    """Random candidates; query i is a random candidate with i % 40 bits flipped (every small distance, many equal ones),
    one query in 50 is random (no close candidate)."""
    rng = np.random.default_rng(100_003 * n1 + n2)
    desc2 = rand_desc(rng, n2)
    desc1 = flip_bits(desc2[rng.integers(0, n2, size=n1)], np.arange(n1) % 40, rng)
    lone = np.arange(n1) % 50 == 49
    desc1[lone] = rand_desc(rng, int(lone.sum()))
    return desc1, desc2


def tiled_descriptors(n1, n2):
    """40 base descriptors tiled over the whole candidate list: equal distances meet across every split of it."""
    rng = np.random.default_rng(100_003 * n1 + n2 + 1)
    base = rand_desc(rng, 40)
    desc2 = np.tile(base, (n2 // 40 + 1, 1))[:n2]
    q = np.concatenate([base, base ^ np.uint32(1), base ^ np.uint32(3), np.roll(base, 1, axis=0)])
    return np.ascontiguousarray(q[np.arange(n1) * 29 % len(q)]), np.ascontiguousarray(desc2)


def match_descriptors(n1, n2):
    return tiled_descriptors(n1, n2) if (n1, n2) == (33, 130_000) else planted_descriptors(n1, n2)


def clip_descriptors():
    """65 536 queries against 140 000 candidates: the candidate list goes out in splits of at most 65 536 (the 16-bit index
    of the matrix-pipe kernel's key).  Query i's unique best candidate is CLIP_TARGETS[i % 6], at distance 36 .. 40; an
    equal copy of that candidate stands later in the list (for the last index: a copy one bit worse, earlier).
    -> (desc1, desc2, target index per query, distance per query)"""
    rng = np.random.default_rng(65_536)
    desc2 = rand_desc(rng, CLIP_N2)
    for t, c in zip(CLIP_TARGETS, CLIP_COPIES):
        if c is not None:
            desc2[c] = desc2[t]
    desc2[CLIP_DECOY] = desc2[CLIP_TARGETS[-1]]
    which = np.arange(CLIP_N1) % len(CLIP_TARGETS)
    target = np.asarray(CLIP_TARGETS)[which]
    dist = 40 - (np.arange(CLIP_N1) // len(CLIP_TARGETS)) % 5
    desc1 = flip_bits(desc2[target], dist, rng)
    # the decoy differs from the last target in one bit, and that target's queries keep this bit as the target has it: they
    # are one bit further from the decoy than from the target
    last = which == len(CLIP_TARGETS) - 1
    bit = np.uint32(1) << np.uint32(5)
    desc1[last, 0] = (desc1[last, 0] & ~bit) | (desc2[CLIP_TARGETS[-1], 0] & bit)
    desc2[CLIP_DECOY, 0] ^= bit
    return desc1, desc2, target, hamming(desc1, desc2[target])


def hamming(a, b):
    """Row-wise Hamming distance of two [n, 8] uint32 arrays."""
    x = np.ascontiguousarray(a ^ b).view(np.uint8)
    return np.unpackbits(x, axis=1).sum(axis=1).astype(np.uint32)


# ---- adjust_contrast restated, and its mutants ----------------------------------------------------------------------------
def stretch_restated(img, mutant=None):
    """orb.rs:455-472 in numpy: f32 coefficient, f32 product, round half away from zero, `as u8`.
    mutant: "half_even" / "truncate" (another rounding of the same f32 product), "f64" (the coefficient and the product in f64)."""
    img = np.asarray(img, dtype=np.uint8)
    lo, hi = int(img.min()), int(img.max())
    if lo >= hi:
        return img.copy()
    v = img.astype(np.int64) - lo
    if mutant == "f64":
        x = (255.0 / float(hi - lo)) * v.astype(np.float64)
    else:
        coeff = np.float32(255) / np.float32(hi - lo)
        x = (coeff * v.astype(np.float32)).astype(np.float64)  # (the f32 product, widened: exact)
        assert (coeff * v.astype(np.float32)).dtype == np.float32
    if mutant == "half_even":
        r = np.round(x)
    elif mutant == "truncate":
        r = np.floor(x)
    else:
        r = np.floor(x + 0.5)  # x >= 0 and x + 0.5 is exact in f64 for an f32 x below 2^24: half away from zero
    return np.clip(r, 0, 255).astype(np.uint8)


def can_survive(w, h, xy):
    """Necessary for a FAST corner to reach the final list: its 31 x 31 patch lies inside the Some(...) cells of the blurred
    grid (orb.rs:271-339: 5 columns and 10 rows of border, rows below `width` only)."""
    x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    return (x >= 20) & (x + 20 < w) & (y >= 25) & (y + 25 < h) & (y + 15 < w)


def surely_survives(w, h, xy):
    """Sufficient: the patch and every rotated sample (|offset| <= 22 = round(15 sqrt 2) + 1) inside the Some(...) cells."""
    x, y = xy[:, 0].astype(np.int64), xy[:, 1].astype(np.int64)
    return (x >= 27) & (x + 27 < w) & (y >= 32) & (y + 32 < h) & (y + 23 < w)


def fast_set(cvref, stretched):
    """The oracle's FAST corners of an (already stretched) image that can reach the final list, as a set of (x, y)."""
    h, w = stretched.shape
    xy, _ = cvref.orb_fast(stretched)
    return {tuple(p) for p in xy[can_survive(w, h, xy)].tolist()}


# ---- the fixture ------------------------------------------------------------------------------------------------------------
GOLDEN_IMAGES = {"stretch170": lambda: stretch_scene(170), "dim4": lambda: dim_scene(4),
                 "ragged97x203": lambda: ragged_scene(97, 203), "crop128x160": periodic_crop}
GOLDEN_MATCH = ("crop128x160", "ragged97x203")  # queries, candidates
GOLDEN_THRESHOLDS = (32, 64)


def golden_entries(extract, match):
    """The arrays of tests/golden/orb_edges.npz from an extractor img -> (xy, desc) and a matcher
    (xy1, desc1, xy2, desc2, threshold) -> (matches, dist): the oracle's (generator, CPU test) or the device's (GPU test)."""
    out, kp = {}, {}
    for name, make in GOLDEN_IMAGES.items():
        kp[name] = extract(make())
        out[name + "_xy"], out[name + "_desc"] = kp[name]
    (xy1, d1), (xy2, d2) = kp[GOLDEN_MATCH[0]], kp[GOLDEN_MATCH[1]]
    for thr in GOLDEN_THRESHOLDS:
        out[f"match{thr}"], out[f"match{thr}_dist"] = match(xy1, d1, xy2, d2, thr)
    return out
