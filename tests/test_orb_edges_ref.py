"""CPU checks of tests/orb_edge_scenes.py: the scenes reach what they are built to reach, and the oracle (oracle/cvref_orb.c)
is right there - against numpy restatements of adjust_contrast (orb.rs:455-472) and of the stable ranking (orb.rs:76-81), and
against the recorded results in tests/golden/orb_edges.npz."""
from pathlib import Path

import numpy as np
import pytest

import orb_edge_scenes as scenes

GOLDEN = Path(__file__).resolve().parent / "golden" / "orb_edges.npz"


def test_stretch_every_span_every_value(oracle):
    """orb_adjust_contrast == f32 quotient, f32 product, round half away from zero, `as u8` for every span 1..255 and every
    value 0..span, at the lowest and the highest offset the span allows."""
    halves = 0
    for span in range(1, 256):
        for lo in (0, 255 - span):
            img = (lo + np.arange(span + 1)).astype(np.uint8)[None]
            got = oracle.orb_adjust_contrast(img)
            want = scenes.stretch_restated(img)
            assert (got == want).all(), (span, lo, np.flatnonzero(got != want))
            assert got[0, 0] == 0 and got[0, -1] == 255
        coeff = np.float32(255) / np.float32(span)
        prod = (coeff * np.arange(span + 1, dtype=np.float32)).astype(np.float64)
        halves += int((prod - np.floor(prod) == 0.5).sum())
    assert halves > 100  # the f32 products do hit exact halves (e.g. 255 / 6 * 3): the rounding mode is exercised
    for flat in (np.full((4, 4), 9, dtype=np.uint8), np.zeros((3, 5), dtype=np.uint8), np.full((1, 1), 255, dtype=np.uint8)):
        assert (oracle.orb_adjust_contrast(flat) == flat).all()  # min >= max: untouched (orb.rs:464-466)


def test_stretch_scenes_have_their_span():
    for span in range(1, 256):
        img = scenes.stretch_scene(span)
        assert img.shape == scenes.STRETCH_SHAPE and int(img.max()) - int(img.min()) == span


@pytest.mark.parametrize("span", scenes.MUTANT_SPANS)
def test_stretch_mutants_change_the_corner_set(oracle, span):
    """A stretch that rounds halves to even or truncates - and at span 200 one with an f64 coefficient - gives other FAST
    corners on stretch_scene(span), among those that can reach the final list: a device stretch that is wrong in one of these
    ways cannot give the oracle's keypoints."""
    img = scenes.stretch_scene(span)
    right = oracle.orb_adjust_contrast(img)
    assert (right == scenes.stretch_restated(img)).all()
    base = scenes.fast_set(oracle, right)
    assert len(base) > 100
    changed = {}
    for mutant in ("half_even", "truncate", "f64"):
        other = scenes.stretch_restated(img, mutant)
        changed[mutant] = len(base ^ scenes.fast_set(oracle, other))
    print(f"span {span}: corners {len(base)}, changed by mutants {changed}")
    assert max(changed["half_even"], changed["truncate"]) > 0, changed
    if span == 200:
        assert changed["f64"] > 0, changed


@pytest.fixture(scope="module")
def periodic(oracle):
    img = scenes.periodic_scene()
    fast_xy, _ = oracle.orb_fast(oracle.orb_adjust_contrast(img))
    resp = [oracle.orb_harris(img, int(x), int(y)) for x, y in fast_xy]
    has = np.array([r is not None for r in resp])
    return img, fast_xy[has], np.array([r for r in resp if r is not None]), oracle.orb_extract(img)


def test_periodic_scene_ties_at_the_cut(periodic):
    img, xy, resp, (out_xy, _) = periodic
    h, w = img.shape
    assert len(resp) > 10_000 and len(np.unique(resp)) < 1000
    order = np.argsort(-resp, kind="stable")  # descending; equal responses keep the scan order of the FAST list
    ranked = resp[order]
    assert ranked[9_999] == ranked[10_000]  # the cut at MAX_KEYPOINTS falls inside a group of equal responses
    top = xy[order[:10_000]]
    # the oracle's list is that ranking minus what extract_brief_descriptors drops at the borders, order kept
    out = {tuple(p) for p in out_xy.tolist()}
    assert len(out) == len(out_xy) > 5000
    kept = np.array([tuple(p) in out for p in top.tolist()])
    assert kept.sum() == len(out_xy) and (top[kept] == out_xy).all()
    assert not kept[~scenes.can_survive(w, h, top)].any()
    assert kept[scenes.surely_survives(w, h, top)].all()
    # ... and inside every group of equal responses it is in scan order
    of = {tuple(p): r for p, r in zip(xy.tolist(), resp.tolist())}
    r_out = np.array([of[tuple(p)] for p in out_xy.tolist()])
    pos = out_xy[:, 1].astype(np.int64) * w + out_xy[:, 0]
    same = r_out[1:] == r_out[:-1]
    assert same.sum() > 5000 and (np.diff(pos)[same] > 0).all() and (np.diff(r_out) <= 0).all()


def test_dim_scenes(oracle):
    two = scenes.dim_scene(2)
    assert set(np.unique(two)) == {0, 1}
    xy, desc = oracle.orb_extract(two)
    assert len(xy) > 100 and (desc == 0).all()  # m00 = 0: NaN orientation, every offset `NaN as isize` = 0
    blur = oracle.orb_gaussian_blur(two)
    assert np.isfinite(blur).sum() > 10_000 and np.nanmax(blur) < 1.0
    four = scenes.dim_scene(4)
    assert set(np.unique(four)) == {0, 1, 2, 3}
    xy, desc = oracle.orb_extract(four)
    assert len(xy) > 300 and (desc != 0).any()
    b4 = oracle.orb_gaussian_blur(four)
    assert np.nanmin(b4) < 1.0 < 2.0 < np.nanmax(b4)  # the patch values truncate to 0, 1 and 2


def test_ragged_scene_counts(oracle):
    for w, h in scenes.RAGGED_SIZES:
        n = len(oracle.orb_extract(scenes.ragged_scene(w, h))[0])
        assert (n > 30) == ((w, h) in scenes.RAGGED_WITH_KEYPOINTS), (w, h, n)
    assert any(w % 4 and (w * h) % 4 for w, h in scenes.RAGGED_SIZES)
    assert len(oracle.orb_extract(scenes.rich_scene())[0]) > 1000
    assert len(oracle.orb_extract(scenes.flat_scene())[0]) == 0


def test_clip_descriptors_are_what_they_claim():
    """The expected result of the 65 536 x 140 000 case is known by construction: check the construction where that is cheap."""
    desc1, desc2, target, dist = scenes.clip_descriptors()
    assert len(desc1) == scenes.CLIP_N1 and len(desc2) == scenes.CLIP_N2
    assert dist.max() == 40 and dist.min() >= 35 and (dist == 40).sum() > 10_000
    for t, c in zip(scenes.CLIP_TARGETS, scenes.CLIP_COPIES):
        if c is not None:
            assert c > t and (desc2[c] == desc2[t]).all()
    last = target == scenes.CLIP_TARGETS[-1]
    decoy = np.broadcast_to(desc2[scenes.CLIP_DECOY], desc1[last].shape)
    assert (scenes.hamming(desc1[last], decoy) == dist[last] + 1).all()
    # a sample of queries against ALL candidates: the target is the first minimum
    for q in range(0, scenes.CLIP_N1, 4099):
        d = scenes.hamming(np.broadcast_to(desc1[q], desc2.shape), desc2)
        assert int(np.argmin(d)) == target[q] and d[target[q]] == dist[q]


def test_oracle_equals_golden_fixture(oracle):
    want = np.load(GOLDEN)
    got = scenes.golden_entries(oracle.orb_extract, oracle.match_points)
    assert sorted(want.files) == sorted(got)
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape and (v == want[k]).all(), k
    assert len(got["match32"]) > 100 and len(got["match64"]) > len(got["match32"])
