"""What the frames of tests/lsd_grow_frames.py make LSD region growing, the rectangle fits and the refinement do -- asserted on the oracle's census
(oracle/lsd_restated.hpp LsdCensus), without a GPU.  tests/test_gpu_lsd_grow.py compares the device growers with the oracle on these frames; the
assertions here are what lets it say which of the growers' branches those comparisons reach.  The census is taken in the stable seed order, the one
most of the GPU comparisons run in.

Every item the growers' structure asks for is asserted below.  Of the ones that frames might not have reached, found and asserted:
  * a regrowth tolerance tau outside [0.01, 1.5): tau = 0 exactly, on the upright bricks (all points near the seed have the seed's angle); no tau >= 1.5
    and no NaN was met: tau is twice a standard deviation of angles that all lie within 22.5 degrees of the region's angle, the largest seen is 0.49;
  * a shrink pass that keeps every point (n_kept == n_before), on the slanted gratings;
  * shrink passes with 64 < n_moves <= 128 and with n_moves > 128 (up to 357), on the slanted gratings.
Not found:
  * a region shrunk below 2 points: the dropped regions of these frames are all dropped by a regrowth that keeps the seed alone (n_regrown < 2), the
    smallest n_kept of any pass is asserted in test_dropped_regions;
  * a kept region whose LAST shrink pass has more than 64 moves: the largest is 47 (194 points before, 147 kept, on a slanted grating).  The
    passes with hundreds of moves are early passes of regions that are shrunk 10 and more times.  What a pass keeps is the set of points within
    its radius whatever the earlier passes did to the list, so those early passes reach the outputs through the density that decides on the next
    pass, and through the order of the f64 sums, not through the kept set: a build whose sequential form skipped the re-examination of a pulled-in
    point passed every comparison of tests/test_gpu_lsd_grow.py (profiles/r25_lsd_grow_paths.md).  Ramp-filled serpentines and V-shaped soft
    edges were tried as well (15 and 31 moves in a last pass);
  * frontier_max7 > 256, the fallback from the 256-word frontier ring to the list in memory.  A region's extent along its gradient is bounded by
    255 / (6 cos 22.5 deg) = 46 half-resolution pixels with 8-bit input, and a frontier is a breadth-first front across such a band: the largest
    value over all frames of the module is 110 (the 45-degree ramp band at the base size; 53 in the 600 x 800 band, 74 on the gratings' webs).
    test_the_frontier_stays_inside_the_ring asserts that it stays at or below 256, so that a frame that does reach the fallback shows up here."""
import os

import numpy as np
import pytest

import lsd_grow_frames as F
import oracle_lib as O

_REF2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "_ref", "libplpref2.so")
FRAMES = F.all_frames()
IDS = [f"{fam}: {name}" for fam, name, _ in FRAMES]


def census(i):
    return F.oracle(i, True).census


def fitted_sizes():
    """every size a rectangle is fitted to: first growths that reached min_reg_size, regrowths and the kept counts of shrink passes, of at least 2 points"""
    s = np.concatenate([np.concatenate([census(i).n_first, census(i).n_regrown[census(i).refined == 1], census(i).n_kept]) for i in range(len(FRAMES))])
    return s[s >= 2]


@pytest.mark.skipif(not os.path.exists(_REF2), reason="oracle/_ref not built (needs /root/reference)")
def test_oracle_equals_the_reference_lsd_on_every_frame():
    """the reference's own LSDDetectorC::detect (std::sort seed order) against the oracle: every key line record"""
    total = 0
    for i, (fam, name, img) in enumerate(FRAMES):
        want = O.ref_lsd_keylines(img)
        got = F.oracle(i, False).all_kl
        assert len(got) == len(want), f"{fam}: {name}: {len(got)} key lines, the reference {len(want)}"
        for k in got.dtype.names:
            if k != "angle":
                assert np.array_equal(got[k], want[k]), f"{fam}: {name}: {k} differs from the reference's"
        # definition D2 (oracle/line_oracle.cpp): the reference's atan2f against the rounded f64 atan2, one unit in the last place at the most
        assert np.all(np.abs(got["angle"] - want["angle"]) <= np.spacing(np.abs(want["angle"]))), f"{fam}: {name}: angle differs from the reference's by more than an ulp"
        total += len(want)
    assert total > 1000


def test_the_census_changes_nothing_and_adds_up():
    for i in (0, 30, len(FRAMES) - 1):
        plain, full = O.LineOracle(FRAMES[i][2], stable_order=True), F.oracle(i, True)
        assert plain.census is None
        for k in ("raw", "all_kl", "all_lbd", "keylsd", "lbd", "linefn", "order", "scaled"):
            assert np.array_equal(getattr(plain, k), getattr(full, k)), f"{IDS[i]}: {k} differs with the census attached"
    for i in range(len(FRAMES)):
        c = census(i)
        assert c.regions_grown >= len(c.n_first) and c.pixels_first >= c.n_first.sum() + (c.regions_grown - len(c.n_first)), IDS[i]
        assert c.kept.sum() == len(F.oracle(i, True).raw), IDS[i]
        assert c.n_passes.sum() == len(c.n_before) and np.array_equal(np.bincount(c.pass_region, minlength=len(c.n_first)), c.n_passes), IDS[i]
        assert np.all(c.n_kept <= c.n_before) and np.all(c.n_moves <= np.minimum(c.n_kept, c.n_before - c.n_kept)), IDS[i]
        assert np.all(c.frontier_max7 <= c.frontier_max) and np.all(c.frontier_max <= np.maximum(c.n_first, c.n_regrown)), IDS[i]
        assert np.all(c.n_regrown[c.refined == 0] == 0) and np.all(c.n_passes[c.refined == 0] == 0), IDS[i]


def test_fit_sizes_cover_the_five_classes_and_both_sides_of_each_threshold():
    """rect_from_ring holds 64 points per register round: <= 64, 65-128, 129-192, 193-256 points, and the general fit above 256"""
    s = fitted_sizes()
    for lo, hi in ((1, 64), (65, 128), (129, 192), (193, 256), (257, 1 << 30)):
        assert np.any((s >= lo) & (s <= hi)), f"no fitted region of {lo}..{hi} points"
    for t in (64, 128, 192, 256):
        assert np.any((s <= t) & (s > t - 8)), f"no fitted size within 8 below {t}"
        assert np.any((s > t) & (s <= t + 8)), f"no fitted size within 8 above {t}"
    small = s[s <= 256]     # the sizes the fit from the ring takes: 32-point chunks and 8-addend batches with their tails
    assert {0, 1, 31} <= set((small % 32).tolist()), sorted(set((small % 32).tolist()))
    assert set((small % 8).tolist()) == set(range(8))


def test_refinement_branches():
    both = [IDS[i] for i in range(len(FRAMES)) if np.any((census(i).kept == 1) & (census(i).refined == 1)) and np.any((census(i).kept == 1) & (census(i).refined == 0))]
    assert both, "no frame with refined and unrefined kept regions"
    passes = np.concatenate([census(i).n_passes[census(i).refined == 1] for i in range(len(FRAMES))])
    assert np.any(passes == 0), "no refined region that needs no shrink pass"
    assert np.any(passes == 1) and np.any(passes == 2) and np.any(passes >= 3), np.bincount(passes).tolist()


def test_dropped_regions():
    """which way regions are dropped in refinement on these frames: by a regrowth of fewer than 2 points; no shrink pass ends below 2"""
    dropped = sum(int(((census(i).refined == 1) & (census(i).kept == 0)).sum()) for i in range(len(FRAMES)))
    by_regrowth = sum(int(((census(i).refined == 1) & (census(i).n_regrown < 2)).sum()) for i in range(len(FRAMES)))
    n_kept = np.concatenate([census(i).n_kept for i in range(len(FRAMES))])
    by_shrink = int((n_kept < 2).sum())
    assert by_regrowth >= 10 and dropped == by_regrowth + by_shrink, (dropped, by_regrowth, by_shrink)
    assert by_shrink == 0 and n_kept.min() >= 2, "a shrink pass now ends below 2 points: say so in the docstring, it is a branch of its own"


def test_regrowth_tolerances():
    tau = np.concatenate([census(i).tau[census(i).refined == 1] for i in range(len(FRAMES))])
    assert np.count_nonzero((tau >= 0.01) & (tau < 1.5)) >= 20
    assert np.any(tau < 0.01), f"no tau below the guard band's range: smallest {tau.min()}"
    assert not np.any(np.isnan(tau)) and tau.max() < 1.5, "a NaN or a tau of 1.5 and more: a sought branch is reached, assert it"


def test_shrink_passes():
    n_before = np.concatenate([census(i).n_before for i in range(len(FRAMES))])
    n_kept = np.concatenate([census(i).n_kept for i in range(len(FRAMES))])
    n_moves = np.concatenate([census(i).n_moves for i in range(len(FRAMES))])
    assert np.any(n_kept == n_before), "no shrink pass that keeps every point (the early return of reduce_radius_pass)"
    assert np.any(n_moves == 0) and np.any((n_moves > 0) & (n_moves <= 64)), "no pass with up to 64 moves (paired moves through the ring, both kernels)"
    assert np.any((n_moves > 64) & (n_moves <= 128)), "no pass with 65..128 moves (paired in k_lsd_grow, sequential in k_lsd_grow_mw)"
    assert np.any(n_moves > 128), "no pass with more than 128 moves (sequential in both kernels)"
    assert np.any(n_kept > 256) and np.any(n_kept <= 256), "shrunk regions on both sides of the fit from the ring"
    # the last pass of a kept region is the one whose kept set reaches the output: its moves go through the paired form (see the module docstring)
    last = [int(census(i).n_moves[np.nonzero(census(i).pass_region == r)[0][-1]]) for i in range(len(FRAMES))
            for r in np.nonzero((census(i).n_passes > 0) & (census(i).kept == 1))[0]]
    assert 32 < max(last) <= 64, f"most moves in a last pass: {max(last)}; above 64 the sequential form decides an output: say so in the docstring"


def test_the_frontier_stays_inside_the_ring():
    fm7 = max(int(census(i).frontier_max7.max(initial=0)) for i in range(len(FRAMES)))
    fm = max(int(census(i).frontier_max.max(initial=0)) for i in range(len(FRAMES)))
    assert 64 < fm7 <= fm <= 256, (fm7, fm)


def test_large_and_small_regions():
    big = [i for i, (fam, _, _) in enumerate(FRAMES) if fam == "big ramp"]
    assert len(big) == 1 and FRAMES[big[0]][2].shape == F.BIG_SHAPE and census(big[0]).n_first.max() > 16384
    assert max(census(i).regions_upto8 for i in range(len(FRAMES)) if FRAMES[i][2].shape == F.SHAPE) >= 1000
    grid = [i for i, (fam, _, _) in enumerate(FRAMES) if fam == "square grid"]
    assert len(grid) == 1 and FRAMES[grid[0]][2].shape == F.GRID_SHAPE and len(F.oracle(grid[0], True).raw) > 2048 and len(F.oracle(grid[0], False).raw) > 2048
    others = [IDS[i] for i in range(len(FRAMES)) if i != grid[0] and len(F.oracle(i, True).raw) >= 2048]
    assert not others, others
    sizes = {img.shape for fam, _, img in FRAMES if fam not in ("big ramp", "square grid", "seed groups")}
    assert sizes == {F.SHAPE} and tuple(F.families()) == F.FAMILY_NAMES
    batch = [len(O.LineOracle(img, stable_order=True).raw) > 2048 for _, img in F.grid_batch_frames()]
    assert batch == [False, True, False], "the overflow batch of the GPU test: only its middle frame overflows"


def test_border_frames_touch_every_border():
    """segments that end within 3 px of each border and each corner: their regions' 3 x 3 neighbourhoods are clipped by the image"""
    h, w = F.SHAPE
    raw = np.concatenate([F.oracle(i, True).raw for i, (fam, _, _) in enumerate(FRAMES) if fam == "borders"]).reshape(-1, 2)
    x, y = raw[:, 0], raw[:, 1]
    left, right, top, bottom = x < 3, x > w - 4, y < 3, y > h - 4
    for name, m in (("left", left), ("right", right), ("top", top), ("bottom", bottom), ("top left", left & top), ("top right", right & top),
                    ("bottom left", left & bottom), ("bottom right", right & bottom)):
        assert np.any(m), f"no segment ends at the {name}"


def test_seed_group_shapes():
    for rem, shape in F.SEED_GROUP_SHAPES.items():
        sh, sw = F.half_size(shape)
        assert (sw - 1) * (sh - 1) % 64 == rem, (shape, sw, sh)
    assert [img.shape for fam, _, img in FRAMES if fam == "seed groups"] == list(F.SEED_GROUP_SHAPES.values())
    for i, (fam, _, img) in enumerate(FRAMES):
        if fam == "seed groups":
            assert F.oracle(i, True).scaled.shape == F.half_size(img.shape) and len(F.oracle(i, True).raw) > 10
