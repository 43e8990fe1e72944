"""The definition of the surface subset (tests/ref_subset.py) on its own, no GPU: known key values, distinct
keys, the shape of the selection, and that the kept set is uniform over the rows and over the pairs of rows."""
import numpy as np
import pytest

import ref_subset

KNOWN = [(0, 0, 0xE220A8397B1DCDAF),  # splitmix64's published first output for seed 0
         (0, 1, 0x6E789E6AA1B965F4),
         (1, 0, 0xBFEF8030DDC2D772),
         (3, 12345, 0x61826B6F5600F3A5),
         (2**64 - 1, 2**32 + 7, 0x28EC8F70181C31E1)]


def test_python_constants_are_the_headers():
    """triangulation.SUBSET_* mirror CVHIP_SUBSET_* (the GPU tests take their shapes from them)."""
    import re
    from pathlib import Path

    from cybervision_amd import triangulation

    text = (Path(__file__).resolve().parent.parent / "include" / "cvhip.h").read_text()
    header = {k: int(v) for k, v in re.findall(r"#define CVHIP_SUBSET_(\w+) (\d+)", text)}
    assert header == {"WG_ROWS": triangulation.SUBSET_WG_ROWS, "GRID_ROWS": triangulation.SUBSET_GRID_ROWS}
    assert header["GRID_ROWS"] % header["WG_ROWS"] == 0 and header["GRID_ROWS"] < 2**20


@pytest.mark.parametrize("seed,i,want", KNOWN)
def test_known_keys(seed, i, want):
    assert ref_subset.key(seed, i) == want
    if i < 20000:
        assert int(ref_subset.keys(i + 1, seed)[i]) == want


def test_keys_of_one_seed_are_distinct():
    for seed in (0, 1, 2**64 - 1):
        assert len(np.unique(ref_subset.keys(1 << 16, seed))) == 1 << 16


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_rows_ascending_unique_and_counted(n):
    for m in (0, 1, 2, n // 2, n - 1, n, n + 1):
        rows = ref_subset.subset_rows(n, m, 5)
        assert rows.dtype == np.uint64 and len(rows) == min(n, m)
        assert (np.diff(rows.astype(np.int64)) > 0).all() and (rows < n).all()


def test_subsets_of_one_seed_are_nested():
    n = 500
    prev = set()
    for m in range(n + 1):
        cur = set(int(r) for r in ref_subset.subset_rows(n, m, 11))
        assert prev <= cur and len(cur) == m
        prev = cur


def test_identity_and_empty():
    assert ref_subset.subset_rows(37, 37, 2).tolist() == list(range(37))
    assert ref_subset.subset_rows(37, 1000, 2).tolist() == list(range(37))
    assert len(ref_subset.subset_rows(37, 0, 2)) == 0
    assert len(ref_subset.subset_rows(0, 5, 2)) == 0


def test_select_smallest_ties_take_the_lower_row():
    k = np.full(100, 7, dtype=np.uint64)
    for m in (0, 1, 50, 99, 100, 101):
        assert ref_subset.select_smallest(k, m).tolist() == list(range(min(m, 100)))
    k = np.array([5, 1, 5, 1, 5, 0], dtype=np.uint64)
    assert ref_subset.select_smallest(k, 4).tolist() == [0, 1, 3, 5]
    assert ref_subset.select_smallest(k, 2).tolist() == [1, 5]


def test_kept_set_is_uniform():
    """n = 64, m = 16, seeds 0 .. 4095.  A row is kept with probability 1/4: its count over the seeds is Binomial(4096, 1/4),
    mean 1024, sigma 27.7, bound 6 sigma = 166.  A pair of rows is kept with probability 16 * 15 / (64 * 63) = 0.05952: mean
    243.8, sigma 15.1, bound 6 sigma = 91."""
    n, m, seeds = 64, 16, 4096
    kept = np.zeros((seeds, n), dtype=np.int64)
    for seed in range(seeds):
        kept[seed, ref_subset.subset_rows(n, m, seed).astype(np.int64)] = 1
    assert (kept.sum(axis=1) == m).all()
    single = kept.sum(axis=0)
    print("inclusion counts", single.min(), single.max())
    assert (np.abs(single - 1024) <= 166).all()
    joint = kept.T @ kept
    pairs = joint[np.triu_indices(n, 1)]
    print("pair counts", pairs.min(), pairs.max())
    assert (np.abs(pairs - 243.8) <= 91).all()
