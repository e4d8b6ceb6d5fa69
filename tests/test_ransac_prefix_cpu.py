"""The sample generator the RANSAC solvers share (csrc/ransac.hpp) without a GPU: step k of the shuffle depends on
(seed, p, iter) and k alone, so for equal (seed, p, iter, n) the three draws of sim3 are the first three of pnp's four, and those the first
four of essential's eight.  A solver whose copy of the shuffle slipped in one index would still return distinct indices in range."""
import numpy as np
import pytest

from plp import plp


@pytest.mark.parametrize("n", [8, 9, 64, 257, 8192])
def test_draws_of_fewer_samples_are_a_prefix(n):
    for seed in (0, 1, 2024, 2**64 - 1):
        for p in (0, 1, 65535):
            d3, d4, d8 = (f(seed, p, 4, n, iter0=1021) for f in (plp.model_sim3_draw, plp.model_pnp_draw, plp.model_essential_draw))
            assert d3.shape == (4, 3) and d4.shape == (4, 4) and d8.shape == (4, 8)
            assert np.array_equal(d3, d4[:, :3]) and np.array_equal(d4, d8[:, :4])
            assert d8.min() >= 0 and d8.max() < n and all(len(set(row)) == 8 for row in d8.tolist())
