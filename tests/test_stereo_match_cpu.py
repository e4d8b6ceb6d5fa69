"""match::stereo::compute on built key points without a GPU: the restatement with reasons (tests/stereo_match_ref.py) against the oracle and,
where it was built, against the reference's own stereo.cc, bit for bit on every scene of tests/stereo_match_scene.py; and the census that holds
the scenes to taking every reachable decision.  The census is a condition on the INPUTS, read off the restatement, never off the kernel."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import stereo_match_ref as R
import stereo_match_scene as S

needs_ref = pytest.mark.skipif(not O.ref2_path().exists(), reason="oracle/_ref/libplpref2.so not built (needs the reference checkout; oracle/ref_build.sh)")
MAIN_NAMES = tuple(c[0] for c in S.MAIN)
OFF_NAMES = tuple(c[0] for c in S.OFF_LEVEL)


def restate(sc):
    return R.compute(sc.levels_l, sc.levels_r, sc.kl, sc.kr, sc.dl, sc.dr, sc.sf, sc.isf, sc.fxb, sc.tb)


@functools.lru_cache(maxsize=None)
def run(name):
    return restate(S.scene(name))


@functools.lru_cache(maxsize=None)
def median_cases():
    sc = S.noise_with_forced_pairs()
    full = restate(sc)
    return sc, full, [(n, sub, restate(sub)) for n, sub in S.median_subsets(sc, full["corr"])]


@functools.lru_cache(maxsize=None)
def single_row():
    lists, want = S.single_row_lists(S.scene("160x208"))
    sc = S.scene("160x208").with_lists(*lists)
    return sc, restate(sc), want


def all_problems():
    for name in S.NAMES:
        yield name, S.scene(name), run(name)
    yield "single row", single_row()[0], single_row()[1]
    sc, full, subs = median_cases()
    yield "noise+forced", sc, full
    for n, sub, r in subs:
        yield f"median/{n}", sub, r


def test_restatement_equals_the_oracle_on_every_scene():
    for name, sc, r in all_problems():
        wx, wd = O.stereo_compute(sc.ol, sc.orr, sc.kl, sc.kr, sc.dl, sc.dr, sc.fxb, sc.tb)
        assert np.array_equal(r["x_right"], wx) and np.array_equal(r["depth"], wd), name
        ok = np.isin(r["reason"], (R.ACCEPTED, R.CLAMPED))
        assert np.array_equal(ok, wx >= 0) and np.array_equal(ok, wd > 0), name


@needs_ref
def test_restatement_equals_the_reference_build_on_every_scene():
    for name, sc, r in all_problems():
        gx, gd = O.ref_stereo_compute(sc.levels_l, sc.levels_r, sc.kl, sc.kr, sc.dl, sc.dr, sc.sf, sc.isf, sc.fxb, sc.tb)
        assert np.array_equal(r["x_right"], gx) and np.array_equal(r["depth"], gd), name


def test_built_frames_and_lists_are_what_the_recipe_says():
    for name, rows, cols, levels, scale, fxb, tb in S.MAIN + S.OFF_LEVEL:
        sc = S.scene(name)
        assert (sc.rows, sc.cols, sc.levels) == (rows, cols, levels) and 120 <= rows <= 288 and 160 <= cols <= 400
        assert np.isclose(sc.sf[1] if levels > 1 else scale, scale) and sc.fxb / sc.tb == fxb / tb
        assert 150 <= len(sc.kl) <= 450 and len(sc.kr) > 64                      # more right key points than one 64-lane pass
        S.assert_legal(sc.kl, sc.sf, rows, cols); S.assert_legal(sc.kr, sc.sf, rows, cols)
        d = [S.disparity_of_row(y, rows) for y in range(rows)]
        assert set(d) >= {0, -3} and min(v for v in d if v > 0) >= 1 and max(d) <= 11
        mid, cx = rows // 2, cols // 2
        blk = sc.left[mid - 16:mid + 16]
        assert np.array_equal(blk[:, cx - 16:cx], blk[:, cx + 1:cx + 17][:, ::-1]) and np.array_equal(blk, sc.right[mid - 16:mid + 16])
        dup = len(sc.kr) - len(np.unique(np.concatenate([sc.kr.view(np.uint8).reshape(len(sc.kr), -1), sc.dr], axis=1), axis=0))
        assert dup >= 10, (name, dup)                                            # right key points listed twice: exact ties
    with pytest.raises(AssertionError):                                          # the builder refuses a key point that would read outside its level
        S.scene("120x160").with_lists(np.array([S.keypoint(5.0, 60.0, 0, S.scene("120x160").sf)], O.KP_DTYPE), S.scene("120x160").kr,
                                      np.zeros((1, 32), np.uint8), S.scene("120x160").dr)


def test_census_of_the_main_configurations():
    tot = np.zeros(len(R.REASONS), np.int64)
    tied = multi = 0
    for name in MAIN_NAMES:
        r = run(name)
        tot += np.bincount(r["reason"], minlength=len(R.REASONS)); tied += r["n_tied"]; multi += r["n_multi"]
    print("\nmain configurations:", dict(zip(R.REASONS, tot.tolist())), "Hamming ties", tied, "more than one candidate", multi)
    for why in (R.ACCEPTED, R.NO_CANDIDATE, R.HAMMING, R.SLIDE_EDGE, R.NEGATIVE_DISPARITY, R.MAX_DISPARITY, R.CLAMPED, R.MEDIAN_REJECTED):
        assert tot[why] >= 5, R.REASONS[why]      # (the window leaves a level only with a scale factor above 2 under the built margin: the 2.5 scenes)
    assert tied >= 20 and multi >= 100


def test_census_first_minimum_and_both_ends_of_the_slide():
    """what the totals do not show: the tie is won by the EARLIER of two equal right key points, and the slide ends on both sides"""
    later_equal = lo = hi = 0
    for name in MAIN_NAMES:
        sc, r = S.scene(name), run(name)
        for il in np.nonzero(r["best_right"] >= 0)[0]:
            b = int(r["best_right"][il])
            same = np.nonzero((sc.dr == sc.dr[b]).all(1) & (sc.kr == sc.kr[b]))[0]
            later_equal += bool((same > b).any())
            assert not (same < b).any()
        for il in np.nonzero(r["reason"] == R.SLIDE_EDGE)[0]:
            kp, b = sc.kl[il], int(r["best_right"][il])
            o = int(kp["octave"])
            isf = np.float32(sc.isf[o])
            sxl, syl, sxr = R.cv_round(kp["x"] * isf), R.cv_round(kp["y"] * isf), R.cv_round(sc.kr["x"][b] * isf)
            pl = sc.levels_l[o][syl - 5:syl + 6, sxl - 5:sxl + 6].astype(int); pl = pl - pl[5, 5]
            c = []
            for off in range(-5, 6):
                pr = sc.levels_r[o][syl - 5:syl + 6, sxr + off - 5:sxr + off + 6].astype(int)
                c.append(int(np.abs(pl - (pr - pr[5, 5])).sum()))
            lo += c.index(min(c)) == 0; hi += c.index(min(c)) == 10
    assert later_equal >= 20 and lo >= 5 and hi >= 5, (later_equal, lo, hi)


def test_census_single_row_of_65_right_key_points():
    sc, r, want = single_row()
    lo, hi = zip(*[R.rows_of_right_keypoint(k["y"], int(k["octave"]), sc.sf) for k in sc.kr])
    assert len(sc.kr) == 65 and len(set(lo)) == 1 and len(set(hi)) == 1 and r["n_multi"] == 3
    assert r["best_right"].tolist() == [want["A"], want["B"], want["C"]] and r["n_tied"] == 1 and r["reason"][2] == R.HAMMING
    assert R.hamming(sc.dl[1], sc.dr[0]) == R.hamming(sc.dl[1], sc.dr[64]) == 2
    assert r["x_right"][0] != r["x_right"][1] and r["reason"][1] == R.ACCEPTED     # A and B share a position: only the winner tells them apart


@pytest.mark.parametrize("wrong", R.WRONG)
def test_census_a_plausible_slip_changes_the_result(wrong):
    """the decisions are not only taken, they show: each slip of stereo_match_ref.WRONG changes x_right of several key points of the main scenes and the median subsets
    (a tie between two copies of one right key point, for one, would not)"""
    changed = 0
    for sc, right in [(S.scene(name), run(name)) for name in MAIN_NAMES] + [(sub, r) for _, sub, r in median_cases()[2]]:
        r = R.compute(sc.levels_l, sc.levels_r, sc.kl, sc.kr, sc.dl, sc.dr, sc.sf, sc.isf, sc.fxb, sc.tb, wrong=wrong)
        changed += int((r["x_right"] != right["x_right"]).sum())
    print(f"\n{wrong}: {changed} results change")
    assert changed >= 5


@pytest.mark.parametrize("name", OFF_NAMES)
def test_census_window_off_the_level(name):
    r = run(name)
    n = int((r["reason"] == R.WINDOW_OFF_LEVEL).sum())
    print(f"\n{name}: window off the level {n}")
    assert n >= 5


def test_census_identical_eyes():
    r = run("identical")
    ok = np.isin(r["reason"], (R.ACCEPTED, R.CLAMPED))
    print("\nidentical eyes:", dict(zip(R.REASONS, np.bincount(r["reason"], minlength=len(R.REASONS)).tolist())))
    assert ok.sum() >= 50 and (r["corr"][ok] == 0).all() and r["median"] == 0


def test_census_noise_pair():
    r = run("noise")
    c = np.bincount(r["reason"], minlength=len(R.REASONS))
    reached = r["corr"][r["corr"] >= 0]
    print("\nnoise pair:", dict(zip(R.REASONS, c.tolist())), "median", r["median"], "largest correlation", int(reached.max()))
    assert c[R.MEDIAN_REJECTED] >= 20 and c[R.ACCEPTED] + c[R.CLAMPED] >= 100
    assert len(set((reached >> 8).tolist())) >= 8                                 # the high-byte pass selects among many buckets


def test_census_median_subsets():
    sc, full, subs = median_cases()
    assert full["corr"].max() >= 1 << 13                                          # the forced pairs, unrelated patches: beyond high byte 32
    assert [n for n, _, _ in subs] == [1, 2, 33, 34, 16]
    for n, sub, r in subs:
        reached = np.sort(r["corr"][r["corr"] >= 0])
        assert len(reached) == n and (r["corr"] < 0).sum() == 5
        assert r["median"] == reached[n // 2]
        if n == 16:
            assert len(set(reached.tolist())) == 16 and (reached > 2 * reached[8]).sum() == 3 and ((reached > 2 * reached[7]) & (reached <= 2 * reached[8])).sum() == 4
            assert (r["reason"] == R.MEDIAN_REJECTED).sum() == 3
        elif n > 2:
            assert (reached == r["median"]).sum() == 3 and reached[n // 2 - 1] == r["median"]     # the median is shared, and sits inside the tie
            assert len(set((reached >> 8).tolist())) >= 8 and reached.max() >= 1 << 13
            assert 3 <= (r["reason"] == R.MEDIAN_REJECTED).sum() < n // 2
