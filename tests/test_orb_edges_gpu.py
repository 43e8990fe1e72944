"""GPU parity of ORB extraction and the keypoint matcher on the scenes of tests/orb_edge_scenes.py: images whose contrast
stretch really stretches, equal Harris responses at the MAX_KEYPOINTS cut, NaN orientations, sizes around every border, a
caller's `cap` below the count, device-resident outputs, and matcher shapes around the switch between its two kernels and
the seams of the candidate splits.  Every comparison is bit for bit against the CPU oracle (or, for the 65 536 x 140 000
matcher case, against the result its construction fixes); every case also holds the oracle's count to a floor.
tests/test_orb_edges_ref.py shows on the CPU that the scenes reach what they are meant to reach."""
import ctypes as C
import time
from pathlib import Path

import numpy as np
import pytest

import orb_edge_scenes as scenes
from cybervision_amd import _lib, orb, pointmatching

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "orb_edges.npz"
DEFAULT_GUARD = 1e-9


def assert_same(got, want, what=""):
    (got_xy, got_desc), (want_xy, want_desc) = got, want
    assert got_xy.shape == want_xy.shape, f"{what}: {len(got_xy)} keypoints, oracle has {len(want_xy)}"
    assert (got_xy == want_xy).all(), f"{what}: keypoint coordinates / order differ"
    assert got_desc.shape == want_desc.shape and (got_desc == want_desc).all(), f"{what}: BRIEF descriptors differ"


_WANT = {}


def want_of(oracle, key, make):
    """The oracle's keypoints of a scene, computed once per session and left unchanged."""
    if key not in _WANT:
        img = make()
        xy, desc = oracle.orb_extract(img)
        xy.setflags(write=False)
        desc.setflags(write=False)
        _WANT[key] = (img, (xy, desc))
    return _WANT[key]


# ---- the contrast stretch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", range(1, 256, 16))
def test_stretch_every_span_batched(gpu_device, oracle, first):
    """stretch_scene(span) for 16 spans in one cvhip_orb_extract_batch: coeff = 255 / span in f32, the f32 product, round
    half away from zero (contrast_body) decide the FAST corners - hence the keypoints - of every image."""
    spans = list(range(first, min(first + 16, 256)))
    cases = [want_of(oracle, ("stretch", s), lambda s=s: scenes.stretch_scene(s)) for s in spans]
    got = orb.extract_points_batch(gpu_device, [img for img, _ in cases])
    for s, g, (_, want) in zip(spans, got, cases):
        assert len(want[0]) > 30, s
        assert_same(g, want, f"span {s}")


@pytest.mark.parametrize("span", [1, 2] + list(scenes.MUTANT_SPANS) + [255])
def test_stretch_single_extraction(gpu_device, oracle, span):
    img, want = want_of(oracle, ("stretch", span), lambda: scenes.stretch_scene(span))
    assert len(want[0]) > 30
    assert_same(orb.extract_points(gpu_device, img), want, f"span {span}")


# ---- equal Harris responses ----------------------------------------------------------------------------------------------
def _periodic(oracle):
    return want_of(oracle, "periodic", scenes.periodic_scene), want_of(oracle, "crop", scenes.periodic_crop)


def test_periodic_single(gpu_device, oracle):
    """Ranks 9 999 and 10 000 are equal, inside a group of 180: f64_order_key and the stable descending radix sort."""
    (img, want), _ = _periodic(oracle)
    assert len(want[0]) > 5000
    assert_same(orb.extract_points(gpu_device, img), want, "periodic")


def test_periodic_tagged_batch(gpu_device, oracle):
    """[periodic, periodic, crop]: the SAME keys in three images of one batch - the first sort interleaves them, the second
    (image << 28 | rank) must hand every image its own ranks in order."""
    (img, want), (crop, want_crop) = _periodic(oracle)
    assert len(want[0]) > 5000 and len(want_crop[0]) > 500
    got = orb.extract_points_batch(gpu_device, [img, img, crop])
    for g, w, what in zip(got, (want, want, want_crop), ("periodic 0", "periodic 1", "crop")):
        assert_same(g, w, what)


def test_periodic_batch_of_17(gpu_device, oracle):
    """More than 16 images: image by image over the handle's streams, every image with its own sort."""
    (img, want), (crop, want_crop) = _periodic(oracle)
    cases = [(img, want), (crop, want_crop)]
    cases += [want_of(oracle, ("ragged", w, h), lambda w=w, h=h: scenes.ragged_scene(w, h)) for w, h in scenes.RAGGED_SIZES]
    cases += [want_of(oracle, ("stretch", s), lambda s=s: scenes.stretch_scene(s)) for s in (6, 34, 102)]
    cases.append((img, want))
    assert len(cases) == 17 and sum(len(w[0]) for _, w in cases) > 15_000
    got = orb.extract_points_batch(gpu_device, [im for im, _ in cases])
    for i, (g, (_, w)) in enumerate(zip(got, cases)):
        assert_same(g, w, f"image {i} of 17")


# ---- dim images: FAST on the stretched image, everything else on the original ----------------------------------------------
@pytest.mark.parametrize("levels", [2, 4])
def test_dim_scenes_at_every_guard(gpu_device, oracle, levels):
    """levels = 2: m00 = 0, the angle is NaN on the device (guard 1e-9, 0.5: atan2 / sin / cos of NaN, near_half(NaN),
    f64_to_i64_sat(NaN)) and on the host (guard 0: std::atan2 of NaN) - 724 keypoints with all-zero descriptors either way.
    levels = 4: blurred values around 1 and 2, truncated by the moments."""
    img, want = want_of(oracle, ("dim", levels), lambda: scenes.dim_scene(levels))
    assert len(want[0]) > (100 if levels == 2 else 300)
    assert (want[1] == 0).all() == (levels == 2)
    try:
        for guard in (DEFAULT_GUARD, 0.5, 0.0):
            orb.set_orientation_guard(gpu_device, guard)
            assert_same(orb.extract_points(gpu_device, img), want, f"dim {levels}, guard {guard}")
    finally:
        orb.set_orientation_guard(gpu_device, DEFAULT_GUARD)


def test_mixed_batch_partly_redone(gpu_device, oracle):
    """Dim, flat, periodic, low-span, 7 x 7: at guard 0.02 some images of the batch are redone on the host and some not."""
    imgs = scenes.mixed_batch()
    want = [oracle.orb_extract(im) for im in imgs]
    counts = [len(w[0]) for w in want]
    assert counts[1] == 0 and counts[4] == 0 and min(counts[0], counts[2], counts[3], counts[5]) > 100
    try:
        orb.set_orientation_guard(gpu_device, 0.02)
        got = orb.extract_points_batch(gpu_device, imgs)
    finally:
        orb.set_orientation_guard(gpu_device, DEFAULT_GUARD)
    for i, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, f"mixed batch, image {i}")


# ---- small and ragged sizes -----------------------------------------------------------------------------------------------
def test_ragged_sizes_single_and_batched(gpu_device, oracle):
    """Widths and pixel counts that are no multiple of four (minmax_body's dword loads and tail), images smaller than the
    Harris / blur / patch borders (no keypoint), tall images (blurred rows >= width do not exist)."""
    cases = [want_of(oracle, ("ragged", w, h), lambda w=w, h=h: scenes.ragged_scene(w, h)) for w, h in scenes.RAGGED_SIZES]
    for (w, h), (_, want) in zip(scenes.RAGGED_SIZES, cases):
        assert (len(want[0]) > 30) == ((w, h) in scenes.RAGGED_WITH_KEYPOINTS), (w, h)
    for (w, h), (img, want) in zip(scenes.RAGGED_SIZES, cases):
        assert_same(orb.extract_points(gpu_device, img), want, f"{w} x {h}")
    got = orb.extract_points_batch(gpu_device, [img for img, _ in cases])
    for (w, h), g, (_, want) in zip(scenes.RAGGED_SIZES, got, cases):
        assert_same(g, want, f"{w} x {h} in the batch")


# ---- the caller's cap -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [50, 1])
def test_cap_below_the_count(gpu_device, oracle, cap):
    """out_cap = min(cap, count): the first `cap` rows of the full result, single and batched."""
    img, want = want_of(oracle, "rich", scenes.rich_scene)
    crop, want_crop = want_of(oracle, "crop", scenes.periodic_crop)
    assert len(want[0]) > 1000 and len(want_crop[0]) > cap
    head = (want[0][:cap], want[1][:cap])
    assert_same(oracle.orb_extract(img, cap), head, "oracle with cap")
    assert_same(orb.extract_points(gpu_device, img, cap=cap), head, f"cap {cap}")
    got = orb.extract_points_batch(gpu_device, [img, crop, scenes.flat_scene()], cap=cap)
    assert_same(got[0], head, f"cap {cap}, batched")
    assert_same(got[1], (want_crop[0][:cap], want_crop[1][:cap]), f"cap {cap}, batched crop")
    assert len(got[2][0]) == 0


# ---- device-resident outputs ---------------------------------------------------------------------------------------------
def _extract_batch_raw(device, imgs, cap, xy_ptrs, desc_ptrs):
    n = len(imgs)
    arrs = [np.ascontiguousarray(im, dtype=np.uint8) for im in imgs]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    ws = (C.c_uint32 * n)(*[a.shape[1] for a in arrs])
    hs = (C.c_uint32 * n)(*[a.shape[0] for a in arrs])
    pxy, pdesc, counts = (C.c_void_p * n)(*xy_ptrs), (C.c_void_p * n)(*desc_ptrs), (C.c_uint32 * n)()
    _lib.check(_lib.lib().cvhip_orb_extract_batch(device.handle, n, ptrs, ws, hs, cap, pxy, pdesc, counts, _lib.NULL_PROGRESS,
                                                  None), "cvhip_orb_extract_batch")
    return [int(c) for c in counts]


@pytest.mark.parametrize("xy_dev,desc_dev", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("n_images", [2, 17])
def test_orb_outputs_on_the_device(gpu_device, oracle, xy_dev, desc_dev, n_images):
    """cvhip_orb_extract_batch with out_xy / out_desc in device memory (torch tensors): the compaction writes into the
    caller's arrays; both on the device, or one of them only; the one-launch form (2 images) and image by image (17)."""
    import torch

    cases = [want_of(oracle, "rich", scenes.rich_scene), want_of(oracle, "crop", scenes.periodic_crop)]
    cases += [want_of(oracle, ("dim", 4), lambda: scenes.dim_scene(4))] * (n_images - 2)
    cap = 4000
    assert all(100 < len(w[0]) < cap for _, w in cases)
    n = len(cases)
    t_xy = [torch.full((cap, 2), -1, dtype=torch.int32, device="cuda") for _ in range(n)]
    t_desc = [torch.full((cap, 8), -1, dtype=torch.int32, device="cuda") for _ in range(n)]
    h_xy = [np.full((cap, 2), 0xFFFFFFFF, dtype=np.uint32) for _ in range(n)]
    h_desc = [np.full((cap, 8), 0xFFFFFFFF, dtype=np.uint32) for _ in range(n)]
    torch.cuda.synchronize()
    counts = _extract_batch_raw(gpu_device, [im for im, _ in cases], cap,
                                [t.data_ptr() for t in t_xy] if xy_dev else [a.ctypes.data for a in h_xy],
                                [t.data_ptr() for t in t_desc] if desc_dev else [a.ctypes.data for a in h_desc])
    gpu_device.synchronize()
    for i, (_, want) in enumerate(cases):
        xy = t_xy[i].cpu().numpy().view(np.uint32) if xy_dev else h_xy[i]
        desc = t_desc[i].cpu().numpy().view(np.uint32) if desc_dev else h_desc[i]
        assert_same((xy[:counts[i]], desc[:counts[i]]), want, f"image {i}")
        assert (xy[counts[i]:] == 0xFFFFFFFF).all() and (desc[counts[i]:] == 0xFFFFFFFF).all()  # nothing past the count


@pytest.mark.parametrize("n1,n2", [(257, 513), (2048, 2048)])
def test_matcher_inputs_and_outputs_on_the_device(gpu_device, oracle, n1, n2):
    """cvhip_match_points with every array in device memory (both kernels): the host-pointer results, and the oracle's."""
    import torch

    desc1, desc2 = scenes.match_descriptors(n1, n2)
    xy1, xy2 = scenes.coords(n1, n2)
    dev = [torch.from_numpy(a.view(np.int32)).cuda() for a in (xy1, desc1, xy2, desc2)]
    for thr in (48, 256):
        want_m, want_d = oracle.match_points(xy1, desc1, xy2, desc2, thr)
        host_m, host_d = pointmatching.match_points(gpu_device, xy1, desc1, xy2, desc2, thr)
        out_m = torch.full((n1, 4), -1, dtype=torch.int32, device="cuda")
        out_d = torch.full((n1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        n = C.c_uint32(0)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(_lib.lib().cvhip_match_points(gpu_device.handle, p(dev[0]), p(dev[1]), n1, p(dev[2]), p(dev[3]), n2, thr,
                                                 p(out_m), p(out_d), C.byref(n)), "cvhip_match_points")
        gpu_device.synchronize()
        got_m = out_m.cpu().numpy().view(np.uint32)
        got_d = out_d.cpu().numpy().view(np.uint32)
        assert n.value == len(want_m) == len(host_m) > n1 // 2
        assert (got_m[:n.value] == want_m).all() and (got_d[:n.value] == want_d).all()
        assert (host_m == want_m).all() and (host_d == want_d).all()
        assert (got_m[n.value:] == 0xFFFFFFFF).all() and (got_d[n.value:] == 0xFFFFFFFF).all()


# ---- matcher shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", scenes.MATCH_SIZES)
def test_matcher_sizes(gpu_device, oracle, n1, n2):
    """One pair; one past and exactly on the vector kernel's 256-query block and 512-candidate tile; n1 * n2 one step below
    and exactly on 2^22, where the matrix-pipe kernel takes over; there 30 candidates (one padded tile), and 33 queries
    (a workgroup that is mostly padding) against 130 000 tiled candidates (1 016 splits, equal distances in all of them).
    A threshold of 0x4000 sends the matrix-pipe sizes through the vector kernel: the same result, no distance exceeds 256."""
    desc1, desc2 = scenes.match_descriptors(n1, n2)
    xy1, xy2 = scenes.coords(n1, n2)
    got = {}
    for thr in scenes.MATCH_THRESHOLDS:
        want_m, want_d = oracle.match_points(xy1, desc1, xy2, desc2, thr)
        got[thr] = pointmatching.match_points(gpu_device, xy1, desc1, xy2, desc2, thr)
        assert got[thr][0].shape == want_m.shape and (got[thr][0] == want_m).all() and (got[thr][1] == want_d).all(), thr
    assert len(got[256][0]) == n1 and len(got[0][0]) >= 1
    if (n1, n2) in scenes.MATCH_SIZES_MATRIX_PIPE:
        assert n1 * n2 >= 1 << 22
        vec_m, vec_d = pointmatching.match_points(gpu_device, xy1, desc1, xy2, desc2, scenes.VECTOR_KERNEL_THRESHOLD)
        assert vec_m.shape == got[256][0].shape and (vec_m == got[256][0]).all() and (vec_d == got[256][1]).all()
    else:
        assert n1 * n2 < 1 << 22
    if (n1, n2) == (33, 130_000):
        assert (got[256][0][:, 2] < 40).all()  # x2 = the candidate's index: always the first of its 3 250 copies


def test_matcher_split_clip_at_65536(gpu_device):
    """n1 = 65 536, n2 = 140 000: 512 workgroups of queries ask for two splits of 70 016 candidates, clipped to 65 536 so that
    the key's 16-bit candidate index holds (three splits).  Every query's unique best candidate sits at a seam - index
    65 535, 65 536, 65 537, 131 071, 131 072 or 139 999 - at distance 35 .. 40, with an equal copy LATER in the list (for
    139 999, which has no later place: a copy one bit worse at index 3), so the expected result is known by construction
    (tests/test_orb_edges_ref.py checks the construction).  Thresholds 256 (all match) and 39 (the distance-40 queries do
    not).  Measured on the MI355X: 4 ms and 3 ms for the two cvhip_match_points calls (copies included), 0.04 s for
    the whole test."""
    desc1, desc2, target, dist = scenes.clip_descriptors()
    xy1, xy2 = scenes.coords(scenes.CLIP_N1, scenes.CLIP_N2)
    assert set(np.unique(target)) == set(scenes.CLIP_TARGETS) and (dist == 40).sum() > 10_000
    for thr in (256, 39):
        t0 = time.perf_counter()
        got_m, got_d = pointmatching.match_points(gpu_device, xy1, desc1, xy2, desc2, thr)
        print(f"match_points 65 536 x 140 000, threshold {thr}: {time.perf_counter() - t0:.3f} s")
        q = np.flatnonzero(dist <= thr)
        q = q[np.argsort(dist[q], kind="stable")]
        want_m = np.stack([xy1[q, 0], xy1[q, 1], xy2[target[q], 0], xy2[target[q], 1]], axis=1)
        assert len(q) > 40_000 and got_m.shape == want_m.shape, (thr, got_m.shape, want_m.shape)
        assert (got_d == dist[q]).all(), thr
        bad = np.flatnonzero((got_m != want_m).any(axis=1))
        assert len(bad) == 0, (thr, len(bad), got_m[bad[:5]], want_m[bad[:5]])


# ---- the fixture -----------------------------------------------------------------------------------------------------------
def test_device_equals_golden_fixture(gpu_device):
    want = np.load(GOLDEN)
    got = scenes.golden_entries(lambda img: orb.extract_points(gpu_device, img),
                                lambda *a: pointmatching.match_points(gpu_device, *a))
    assert sorted(want.files) == sorted(got)
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape and (v == want[k]).all(), k
    assert len(want["match32"]) > 100 and len(want["crop128x160_xy"]) > 500
