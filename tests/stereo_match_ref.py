"""CPU restatement of match::stereo::compute (match/stereo.cc:45-301) as plp_stereo_compute / plp_stereo_compute_batch_device define it, with the
REASON each left key point ends on: plain Python per key point in the reference's order, numpy.float32 one operation at a time where the
reference computes in float, Python float (f64) where it computes in double, Python int for the SAD.

Two rejections of the reference cannot fire on valid input and have no reason code:
  * `max_x_right < 0` (:76) needs x_left < 0 (min_disp_ is 0), and a key point lies inside the image;
  * `x_delta < -1 || 1 < x_delta` (:292) cannot happen: best_offset is the FIRST STRICT minimum of the eleven correlations and is not at an
    end of the slide, so c1 > c2 and c3 >= c2; with a = c1 - c2 > 0, b = c3 - c2 >= 0 the quotient is (a - b) / (2 (a + b)), and
    |a - b| <= a + b gives |x_delta| <= 1/2 (the denominator 2 (a + b) is positive, so the quotient is finite as well).
compute() asserts both instead.

Legal input (the reference indexes rows with .at() and reads the patches unchecked; so does the kernel): every octave below the number of
levels, floor(y - 2 s) >= 0 and ceil(y + 2 s) < rows for every right key point (s = the scale of its octave), and the 11 x 11 patch of every left
key point inside its level.  compute() asserts what it indexes."""
import numpy as np

f32 = np.float32

ACCEPTED, NO_CANDIDATE, HAMMING, WINDOW_OFF_LEVEL, SLIDE_EDGE, NEGATIVE_DISPARITY, MAX_DISPARITY, CLAMPED, MEDIAN_REJECTED = range(9)
REASONS = ("accepted", "no candidate", "Hamming >= 75", "window off the level", "edge of slide", "negative disparity", "disparity >= max",
           "0.01 clamp", "median rejection")
HAMM_DIST_THR = (100 + 50) // 2          # match/stereo.h: hamm_dist_thr_ = (HAMMING_DIST_THR_HIGH + HAMMING_DIST_THR_LOW) / 2
WIN, SLIDE = 5, 5


def cv_round(v):
    """cvRound(float): round half to even"""
    return int(np.rint(f32(v)))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def rows_of_right_keypoint(y, octave, scale_factors, wrong=None):
    """get_right_keypoint_indices_in_each_row(2.0) (:152-183): the inclusive row range [min_r, max_r] one right key point is listed in"""
    r = f32(f32(2.0) * f32(scale_factors[octave]))
    if wrong == "band_rounded":
        return int(np.rint(f32(f32(y) - r))), int(np.rint(f32(f32(y) + r)))
    return int(np.floor(f32(f32(y) - r))), int(np.ceil(f32(f32(y) + r)))


def subpixel(level_l, level_r, kp_l, x_right, scale_factors, inv_scale_factors):
    """compute_subpixel_disparity (:225-301) -> (reason or None, best_x_right, best_disp, correlation (int), x_delta)"""
    o = int(kp_l["octave"])
    isf = f32(inv_scale_factors[o])
    sxl, syl, sxr = cv_round(f32(kp_l["x"]) * isf), cv_round(f32(kp_l["y"]) * isf), cv_round(f32(x_right) * isf)
    rows, cols = level_r.shape
    if sxr - SLIDE - WIN < 0 or cols <= sxr + SLIDE + WIN:
        return WINDOW_OFF_LEVEL, None, None, None, None                                          # :241-244
    assert WIN <= syl < rows - WIN and WIN <= sxl < level_l.shape[1] - WIN, "the left patch leaves its level: not legal input"
    pl = level_l[syl - WIN:syl + WIN + 1, sxl - WIN:sxl + WIN + 1].astype(np.int64)
    pl = pl - pl[WIN, WIN]                                                                       # :255-256, integers held in float
    corr = []
    for off in range(-SLIDE, SLIDE + 1):
        pr = level_r[syl - WIN:syl + WIN + 1, sxr + off - WIN:sxr + off + WIN + 1].astype(np.int64)
        pr = pr - pr[WIN, WIN]
        corr.append(int(np.abs(pl - pr).sum()))                                                  # cv::norm(NORM_L1): <= 121 * 510, exact in f32
    best = min(range(2 * SLIDE + 1), key=lambda i: (corr[i], i))                                 # `correlation < best_correlation`: first strict minimum
    best_off = best - SLIDE
    if best_off == -SLIDE or best_off == SLIDE:
        return SLIDE_EDGE, None, None, None, None                                                # :278-281
    c1, c2, c3 = f32(corr[best - 1]), f32(corr[best]), f32(corr[best + 1])
    assert c1 > c2 and c3 >= c2
    x_delta = f32(float(f32(c1 - c3)) / (2.0 * float(f32(c1 + c3)) - 4.0 * float(c2)))          # :290: float numerator, double quotient, narrowed
    assert -0.5 <= x_delta <= 0.5
    best_x_right = f32(f32(scale_factors[o]) * f32(f32(sxr + best_off) + x_delta))              # :298
    best_disp = f32(f32(kp_l["x"]) - best_x_right)                                               # :299
    return None, best_x_right, best_disp, corr[best], x_delta


def median_threshold(correlations, wrong=None):
    """(:130-137) -> (median, threshold): sorted(int corr)[n // 2] and float(2.0 * median); (0, 0) for an empty list"""
    c = sorted(int(v) for v in correlations)
    median = f32(c[(len(c) - 1) // 2 if wrong == "lower_median" else len(c) // 2]) if c else f32(0.0)
    return int(median), f32(2.0 * float(median))


WRONG = ("last_minimum", "hamming_74", "hamming_76", "band_rounded", "octave_2", "lower_median")


def compute(levels_l, levels_r, kl, kr, dl, dr, scale_factors, inv_scale_factors, fxb, tb, wrong=None):
    """wrong: None = the reference; one of WRONG = a plausible slip of an implementation (the last minimum instead of the first, the Hamming
    threshold off by one, the row band rounded instead of floor / ceil, octave +-2 let through, the lower median), NOT the reference's result:
    tests/test_stereo_match_cpu.py holds the scenes to telling each of them from the reference.
    -> dict(x_right, depth, reason [n_l], corr [n_l] (the integer correlation of a key point that reached the median step, else -1),
    best_right [n_l] (index of the chosen right key point, -1 without one), x_delta [n_l], median, n_tied (left key points whose minimum Hamming
    distance, below 75, is shared by at least two candidates), n_multi (left key points with more than one candidate)); a candidate is a right
    key point that passes the row, octave and x gates, i.e. one whose Hamming distance the reference computes."""
    n_l, n_r = len(kl), len(kr)
    rows = levels_l[0].shape[0]
    max_disp, min_disp = f32(f32(fxb) / f32(tb)), f32(0.0)
    x_right = np.full(n_l, -1, np.float32); depth = np.full(n_l, -1, np.float32)
    reason = np.full(n_l, NO_CANDIDATE, np.int32); corr = np.full(n_l, -1, np.int64); best_right = np.full(n_l, -1, np.int64)
    x_deltas = np.full(n_l, np.nan, np.float32)
    assert wrong is None or wrong in WRONG
    thr_h = {"hamming_74": HAMM_DIST_THR - 1, "hamming_76": HAMM_DIST_THR + 1}.get(wrong, HAMM_DIST_THR)
    reach = 2 if wrong == "octave_2" else 1
    band = [rows_of_right_keypoint(kr["y"][i], int(kr["octave"][i]), scale_factors, wrong) for i in range(n_r)]
    assert all(0 <= int(o) < len(levels_l) for o in kr["octave"]) and all(0 <= lo and hi < rows for lo, hi in band), "right key point: not legal input"
    lo_r = np.array([b[0] for b in band], np.int64); hi_r = np.array([b[1] for b in band], np.int64)
    n_tied = n_multi = 0
    for il in range(n_l):
        kp = kl[il]
        o = int(kp["octave"])
        assert 0 <= o < len(levels_l) and 0 <= kp["y"] < rows and kp["x"] >= 0, "left key point: not legal input"
        row = int(kp["y"])                                                                       # indices_right_in_row.at(y_left): float -> size_t
        min_x, max_x = f32(f32(kp["x"]) - max_disp), f32(f32(kp["x"]) - min_disp)
        cand = [ir for ir in np.nonzero((lo_r <= row) & (row <= hi_r))[0]                        # in right-index order, as the rows were filled
                if o - reach <= int(kr["octave"][ir]) <= o + reach and not (kr["x"][ir] < min_x or max_x < kr["x"][ir])]
        if not cand:
            continue                                                                             # :68-71 or best_hamm_dist stays 75 (:87-90)
        n_multi += len(cand) > 1
        dist = [hamming(dl[il], dr[ir]) for ir in cand]
        best = min(range(len(cand)), key=lambda i: (dist[i], -i if wrong == "last_minimum" else i))   # `hamm_dist < best_hamm_dist`: the first minimum
        if dist[best] >= thr_h:
            reason[il] = HAMMING
            continue
        n_tied += dist.count(dist[best]) > 1
        best_right[il] = cand[best]
        why, bx, bd, c, xd = subpixel(levels_l[o], levels_r[o], kp, kr["x"][cand[best]], scale_factors, inv_scale_factors)
        if why is not None:
            reason[il] = why
            continue
        x_deltas[il] = xd
        if bd < min_disp:
            reason[il] = NEGATIVE_DISPARITY                                                      # :104
            continue
        if max_disp <= bd:
            reason[il] = MAX_DISPARITY
            continue
        reason[il] = ACCEPTED
        if bd <= f32(0.0):
            bd = f32(0.01); bx = f32(f32(kp["x"]) - bd)                                          # :110-115
            reason[il] = CLAMPED
        depth[il] = f32(f32(fxb) / bd); x_right[il] = bx; corr[il] = c
    median, thr = median_threshold(corr[corr >= 0], wrong)
    for il in np.nonzero(corr >= 0)[0]:
        if thr < f32(corr[il]):                                                                  # :144, int correlation converted to float
            x_right[il] = depth[il] = -1
            reason[il] = MEDIAN_REJECTED
    return dict(x_right=x_right, depth=depth, reason=reason, corr=corr, best_right=best_right, x_delta=x_deltas, median=median, n_tied=int(n_tied),
                n_multi=int(n_multi))
