"""CPU-only: the rank sort that k_quadtree runs on levels of a few hundred candidates (csrc/quadtree_model.hpp qt_rank, the code the kernel
compiles) orders any input like a stable sort by the shifted key -- what the radix passes of the large path produce."""
import numpy as np

from plp import plp


def want(keys, shift):
    return np.argsort(np.asarray(keys, np.uint32) >> np.uint32(shift), kind="stable").astype(np.uint32)


def test_rank_sort_equals_stable_sort_on_random_keys_with_duplicates():
    rng = np.random.default_rng(24)
    sizes = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 409, 440, 511, 512]     # around the four-key reads, the wave's 64 and the path's limits
    for trial in range(300):
        n = sizes[trial % len(sizes)] if trial < 190 else int(rng.integers(0, 513))
        hi = (2, 3, 7, 50, 1 << 12, 1 << 24, 1 << 31)[trial % 7]       # few distinct values -> long runs of equal keys, up to the largest tree key
        keys = rng.integers(0, hi, n, dtype=np.uint64).astype(np.uint32)
        shift = (0, 0, 2, 6, 10)[trial % 5]
        got = plp.model_quadtree_rank_sort(keys, shift)
        assert np.array_equal(got, want(keys, shift)), (trial, n, hi, shift)


def test_rank_sort_corner_inputs():
    for n in (1, 64, 65, 200, 512):
        for keys in (np.zeros(n, np.uint32), np.full(n, 0x7fffffff, np.uint32), np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1].copy(),
                     (np.arange(n, dtype=np.uint32) // 70)[::-1].copy()):      # all equal (smallest and largest key), sorted, reversed, runs that straddle the 64-entry groups
            assert np.array_equal(plp.model_quadtree_rank_sort(keys), want(keys, 0)), (n, keys[:4])
    # bits below the shift must not take part: equal shifted keys keep their input order
    keys = np.array([7, 4, 5, 6, 3, 0, 1, 2] * 40, np.uint32)
    assert np.array_equal(plp.model_quadtree_rank_sort(keys, 2), want(keys, 2))
