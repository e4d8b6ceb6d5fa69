"""The exact seed sort's partitions in global memory hand the stoppers' entries from side to side through an LDS tile of R ranks, tile after tile
(csrc/seed_sort_impl.inc wg_partition, "B / C").  These are the smallest arrays at which that loop can go wrong: one global partition just above each
window, swap counts m at and around the multiples of R, chunks that straddle a tile's border on both sides, a dead right part, many tiles of a frame whose
prefix arrays fill the LDS, forced recursion budgets.  The kernel (plp.seed_introsort_debug) against libstdc++ (oracle) / the host model; R comes from the
library (plp.seed_sort_tile_ranks), and every built array is checked on the CPU -- by libstdc++'s partition restated below -- to make the m it is meant for."""
import numpy as np
import pytest

import oracle_lib as O
from plp import plp
from test_index_models import _seed_entries

HI, LO = 700, 300
WINDOW = {0: 4096, 1: 24576}          # entries of the LDS window of the two kernel configurations (include/plp_front.h, plp_seed_introsort_debug)
N_TILES = {0: 12000, 1: 80000}        # a first partition here can make 2 R + 1 swaps: R falls with the segment's chunks, m is at most half the segment


def _key(e):
    return (np.asarray(e) >> np.uint32(20)).astype(np.int64)


def _entries(keys):
    keys = np.asarray(keys)
    return (keys.astype(np.uint32) << np.uint32(20)) | np.arange(len(keys), dtype=np.uint32)


def _want(e, depth=-1):
    w = O.std_introsort_loop_entries(e, depth)
    return plp.model_seed_introsort(e, depth) if w is None else w


def _first_partition(e):
    """std::__unguarded_partition_pivot on the whole array for keys in descending order (comp(a, b) = key a > key b), restated from the library's text:
    the median of a[1], a[mid], a[n - 1] goes to a[0]; the scans stop at keys <= pivot from the left and >= pivot from the right and swap while they have not met.
    Returns (m = swaps, cut, pivot key, positions of the left stoppers in scan order, of the right stoppers in scan order)."""
    k = _key(e).copy()
    n = len(k)
    mid = n // 2
    a, b, c = 1, mid, n - 1
    gt = lambda i, j: k[i] > k[j]
    if gt(a, b):
        m3 = b if gt(b, c) else (c if gt(a, c) else a)
    else:
        m3 = a if gt(a, c) else (c if gt(b, c) else b)
    k[0], k[m3] = k[m3], k[0]
    pk = int(k[0])
    L = np.flatnonzero(k[1:] <= pk) + 1
    Rr = (np.flatnonzero(k[1:] >= pk) + 1)[::-1]
    q = min(len(L), len(Rr))
    m = int(np.count_nonzero(L[:q] < Rr[:q]))
    assert np.all(L[:m] < Rr[:m])                                     # (the swaps are a prefix of the ranks)
    cut = int(L[0]) if m == 0 else int(min(L[m] if m < len(L) else n, Rr[m - 1]))
    return m, cut, pk, L, Rr


def _two_valued(n, target_m, rng, spread):
    """an array of n entries with keys HI / LO whose first partition makes exactly target_m swaps.  Pivot LO: every entry stops the scan from the right, the LO
    entries stop the one from the left, so m = the LO entries in the left part, give or take the median's own moves -- settled by trying the counts next to the
    target.  spread: the LO entries lie scattered over the first `spread` positions (chunks with few stoppers on the left, full chunks on the right)."""
    mid = n // 2
    if target_m == 0:                 # (a LO pivot always finds a[1] to swap.)  Already parted: HI, then the pivot's own value once, then LO
        keys = np.where(np.arange(n) < mid, HI, LO)
        keys[mid] = (HI + LO) // 2
        return _entries(keys)
    pool = np.setdiff1d(np.arange(2, min(spread, n - 2 - target_m - 8)), [mid])
    for a0 in (HI, LO):
        for cnt in range(max(0, target_m - 3), target_m + 4):
            if cnt > len(pool):
                continue
            keys = np.full(n, HI)
            keys[[1, mid]] = LO
            keys[0] = a0
            keys[rng.choice(pool, cnt, replace=False)] = LO
            e = _entries(keys)
            if _first_partition(e)[0] == target_m:
                return e
    raise AssertionError(("no array with this swap count", n, target_m))


def _check(e, variant, depth=-1):
    got = plp.seed_introsort_debug(e, depth, variant=variant)
    assert np.array_equal(got, _want(e, depth))


def test_every_global_partition_of_every_frame_size_has_an_exchange_tile():
    """no GPU: the tile is what the segment's prefix arrays (and masks) leave of the LDS; the launch grows the LDS with the frame, so a tile is never short"""
    for variant in (0, 1):
        for n in [WINDOW[variant] + 1, 5000, 30000, 76241, 115753, 229401, 400000, 524257]:
            if n <= WINDOW[variant]:
                continue
            for seg in sorted({WINDOW[variant] + 1, (WINDOW[variant] + 1 + n) // 2, n - 1, n}):
                r, lm = plp.seed_sort_tile_ranks(n, seg, variant, return_masks=True)
                assert r >= 64, (variant, n, seg, r, lm)
    assert plp.seed_sort_tile_ranks(76241, 76241, 0, return_masks=True)[1] is False      # a 640 x 480 frame: the first partition's masks stay in HBM ...
    assert plp.seed_sort_tile_ranks(76241, 30000, 0, return_masks=True)[1] is True       # ... a later one's are in LDS
    with pytest.raises(ValueError):
        plp.seed_sort_tile_ranks(100, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_one_global_partition_just_above_the_window(variant):
    """n - window in 1 .. ~120: exactly one partition in global memory (both parts fit the window), of one tile, on every key shape"""
    w = WINDOW[variant]
    r = np.random.default_rng(100 + variant)
    for n in [w + 1, w + 2, w + 63, w + 64, w + 65, w + 104, w + 123]:
        assert plp.seed_sort_tile_ranks(n, n, variant) >= n // 2      # one tile holds every swap
        for kind in range(8):
            _check(_seed_entries(r, n, kind), variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_swap_counts_at_and_around_the_multiples_of_the_tile(variant):
    """m = 0, 1, R - 1, R, R + 1, 2 R, 2 R + 1 (the last tile holds one rank at R + 1 and 2 R + 1), with the left stoppers sparse (a tile spans many chunks on
    the left and few on the right) and dense"""
    n = N_TILES[variant]
    R = plp.seed_sort_tile_ranks(n, n, variant)
    assert 64 <= R and 2 * R + 1 < n // 2 - 16
    rng = np.random.default_rng(200 + variant)
    for m in (0, 1, R - 1, R, R + 1, 2 * R, 2 * R + 1):
        for spread in (n // 2, min(n // 2, m + m // 8 + 80)):
            e = _two_valued(n, m, rng, spread)
            assert _first_partition(e)[0] == m
            _check(e, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_chunks_that_straddle_a_tile_border_on_both_sides(variant):
    """random two-valued keys: stoppers in every chunk of both sides; checked on the CPU that ranks R - 1 and R share a chunk on the left AND on the right"""
    n = N_TILES[variant]
    R = plp.seed_sort_tile_ranks(n, n, variant)
    rng = np.random.default_rng(300 + variant)
    found = 0
    for trial in range(40):
        e = _entries(np.where(rng.random(n) < 0.5, HI, LO))
        m, _, _, L, Rr = _first_partition(e)
        if m <= R + 1 or (L[R - 1] - 1) >> 6 != (L[R] - 1) >> 6 or (Rr[R - 1] - 1) >> 6 != (Rr[R] - 1) >> 6:
            continue
        found += 1
        _check(e, variant)
        if found == 3:
            break
    assert found == 3, found


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_a_dead_first_partition_whose_swaps_are_no_multiple_of_the_tile(variant):
    """pivot key below the skip key and last == n_live: the right stoppers still hand their entries over, nothing is stored into the right part; the live part
    and its length are the model's"""
    n = N_TILES[variant]
    R = plp.seed_sort_tile_ranks(n, n, variant)
    rng = np.random.default_rng(400 + variant)
    skip = (HI + LO) // 2
    for m in (R + R // 2 + 7, 2 * R + 1, 5):
        e = _two_valued(n, m, rng, n // 2)
        got_m, cut, pk, _, _ = _first_partition(e)
        assert got_m == m and m % R != 0 and pk == LO and pk < skip
        got, n_live = plp.seed_introsort_debug(e, -1, skip, variant=variant, return_live=True)
        want = plp.model_seed_introsort(e, -1, skip)
        assert 0 < n_live <= cut < n, (n_live, cut)                   # the first partition's right part [cut, n) is dead
        assert np.array_equal(got[:n_live], want[:n_live])
        assert np.all(_key(want[n_live:]) < skip) and np.count_nonzero(_key(got[:n_live]) >= skip) == np.count_nonzero(_key(e) >= skip)
    # ... and image-like keys with a skip key, where later partitions are dead as well
    for trial in range(4):
        e = _seed_entries(rng, n + trial, [1, 7, 0, 2][trial])
        skip = [20, 25, 500, 1][trial]
        got, n_live = plp.seed_introsort_debug(e, -1, skip, variant=variant, return_live=True)
        want = plp.model_seed_introsort(e, -1, skip)
        assert 0 < n_live <= len(e) and np.array_equal(got[:n_live], want[:n_live]) and np.all(_key(want[n_live:]) < skip), (trial, n_live)


@pytest.mark.gpu
def test_a_frame_whose_prefix_arrays_fill_the_lds_exchanges_through_many_tiles():
    """229 401 entries (a 1241 x 376 frame at scale 0.8) in the 4-wave configuration: the launch grows the LDS for the first partition's prefix arrays, the tile is
    what is left beside them -- some sixty tiles for a two-valued array -- and its masks are in HBM"""
    n = 229401
    R, lm = plp.seed_sort_tile_ranks(n, n, 0, return_masks=True)
    assert not lm and 64 <= R < 4096
    rng = np.random.default_rng(500)
    e = _entries(np.where(rng.random(n) < 0.5, HI, LO))
    assert _first_partition(e)[0] > 8 * R
    _check(e, 0)
    skip = (HI + LO) // 2
    got, n_live = plp.seed_introsort_debug(e, -1, skip, variant=0, return_live=True)
    want = plp.model_seed_introsort(e, -1, skip)
    assert 0 < n_live <= n and np.array_equal(got[:n_live], want[:n_live]) and np.all(_key(want[n_live:]) < skip)
    # the SECOND partition on either side of the length at which a segment's masks move into LDS (prefix arrays, masks and pBi all have to fit beside the tile:
    # pBi has a slot per chunk, more than the smallest tile's bytes at this length): the first cut is set by the number of keys above the pivot
    sizes = [s for s in range(60000, 125000, 1000) if plp.seed_sort_tile_ranks(n, s, 0, return_masks=True)[1] != plp.seed_sort_tile_ranks(n, s + 1000, 0, return_masks=True)[1]]
    assert len(sizes) == 1, sizes
    seen = set()
    for s in (sizes[0] - 3000, sizes[0], sizes[0] + 1000, sizes[0] + 4000):
        keys = rng.integers(0, 512, n)
        keys[rng.choice(np.arange(2, n - 1), s, replace=False)] = rng.integers(513, 1024, s)
        keys[[1, n // 2, n - 1]] = 512
        e = _entries(keys)
        cut = _first_partition(e)[1]
        assert abs(cut - s) <= 8, (cut, s)
        seen.add(plp.seed_sort_tile_ranks(n, cut, 0, return_masks=True)[1])
        _check(e, 0)
    assert seen == {False, True}


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_forced_budgets_end_in_the_heap_sort_after_global_partitions(depth):
    """n about 9 000 in the 4-wave configuration (26 000 in the 16-wave one, budgets above 0): `depth` global partitions, then one lane's heap sort"""
    rng = np.random.default_rng(600 + depth)
    for kind in (0, 1, 2, 6, 7):
        _check(_seed_entries(rng, 9000 + kind, kind), 0, depth)
    if depth:
        for kind in (0, 7):
            _check(_seed_entries(rng, 26000 + kind, kind), 1, depth)
