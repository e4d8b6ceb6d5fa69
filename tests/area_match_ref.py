"""CPU restatement of match::area::match_in_consistent_area (match/area.cc:33-153) as plp_match_area_host defines it, with the REASON each key
point of frame 1 ends on and the facts of a scene that an implementation can get wrong without a random problem noticing.  Plain Python per key
point in the reference's order; numpy.float32 one operation at a time where the reference computes in float, Python float (f64) where it
computes in double.  The arrays are those of oracle_lib.match_area.

The candidates of a key point are visited as get_keypoints_in_cell lists them (data/common.cc:241-313): cell columns ascending, rows ascending
inside a column, indices ascending inside a cell.  The strict `<` updates of best and second (:82-91) then make best the FIRST smallest distance
in that order and second the second smallest of the multiset, i.e. the two smallest (distance, column, row, index) keys.

One step is not restated: which of several equally full bins std::sort ranks first (angle_checker.h:165-176) is the C++ library's business, so
the ranking of the 30 bin sizes is oracle_lib.index_sort_by_size, this machine's std::sort on those sizes.  `rank_bins` can be replaced to see
what another ranking would give."""
import math

import numpy as np

f32 = np.float32

OCTAVE_SKIPPED, WINDOW_OUTSIDE, NO_CANDIDATE, ALL_HELD, BEST_ABOVE_50, RATIO_REJECTED, MATCHED_FRESH, MATCHED_STEALING = range(8)
REASONS = ("octave skipped", "window outside the grid", "no candidate", "every candidate already held at least as closely", "best > 50",
           "ratio rejected", "matched fresh", "matched by stealing")
FACTS = ("same_lane", "different_lanes", "best_equals_second", "tie_won_by_cell_order", "orientation_removals", "bin_tie_at_cut",
         "stolen_entry_changes_bins")
HAMMING_DIST_THR_LOW, MAX_HAMMING_DIST = 50, 256
HIST_LEN, NUM_BINS_THR = 30, 3


def _std_sort_ranking(sizes):
    import oracle_lib as O
    return [int(v) for v in O.index_sort_by_size(np.asarray(sizes, np.int32))]


def angle_bin(a1, a2):
    """angle_checker::append_delta_angle (angle_checker.h): float difference, the two wraps in double narrowed back, cvRound(delta * (1.0f / 30))
    -> (bin, wrapped up from below 0, wrapped down from 360 or more)"""
    delta = f32(f32(a1) - f32(a2))
    up = bool(delta < 0.0)
    if up:
        delta = f32(float(delta) + 360.0)
    down = bool(360.0 <= delta)
    if down:
        delta = f32(float(delta) - 360.0)
    b = int(np.rint(f32(delta * f32(f32(1.0) / f32(HIST_LEN)))))
    assert 0 <= b < HIST_LEN, "hist_.at(bin) would throw: not legal input"
    return b, up, down


def valid_bins(sizes, rank_bins):
    """-> (the NUM_BINS_THR bins that survive, whether ranks 3 and 4 hold equally many (> 0) entries)"""
    order = rank_bins(sizes)
    tie = sizes[order[NUM_BINS_THR]] > 0 and sizes[order[NUM_BINS_THR - 1]] == sizes[order[NUM_BINS_THR]]
    return set(order[:NUM_BINS_THR]), bool(tie)


def match(g6, kps1, desc1, kps2, desc2, prev_pts, margin, ratio, check_orientation, rank_bins=_std_sort_ranking):
    """-> (matched_2_in_1 [n1] i32, prev_matched_pts [n1, 2] f32 (a copy, updated), num_matches, census)

    census: reason [n1]; best_i2 / second_i2 [n1] (the two smallest keys among the candidates not held at least as closely, -1 without one);
    best / second [n1] (their distances, 256 without one); third [n1] (the third smallest distance, 256 without one); clipped [n1] (the window
    was cut at a border of the grid); wrap_up / wrap_down (matches whose angle difference was below 0 / at or above 360 after that);
    nonempty_bins; num_steals; facts: dict over FACTS (counts, or booleans for the last two)."""
    n1, n2 = len(kps1), len(kps2)
    min_x, min_y, inv_w, inv_h, cols, rows = f32(g6[0]), f32(g6[1]), float(g6[2]), float(g6[3]), int(g6[4]), int(g6[5])
    mg, ratio = f32(int(margin)), f32(ratio)
    x2 = np.asarray(kps2["x"], f32); y2 = np.asarray(kps2["y"], f32); o2 = np.asarray(kps2["octave"], np.int64)
    d1 = np.asarray(desc1, np.uint8).reshape(n1, 32); d2 = np.asarray(desc2, np.uint8).reshape(n2, 32)
    # assign_keypoints_to_grid (common.cc:205-231): cvFloor((x - min_x) * inv_cell_width), float difference times double
    cx2 = np.floor((x2 - min_x).astype(np.float64) * inv_w).astype(np.int64); cy2 = np.floor((y2 - min_y).astype(np.float64) * inv_h).astype(np.int64)
    in_grid = (0 <= cx2) & (cx2 < cols) & (0 <= cy2) & (cy2 < rows)

    matched = np.full(n1, -1, np.int32)
    pp = np.array(prev_pts, f32).reshape(n1, 2).copy()
    dists_2 = np.full(n2, MAX_HAMMING_DIST, np.int64); idx1_in_2 = np.full(n2, -1, np.int64)
    num = 0
    reason = np.full(n1, NO_CANDIDATE, np.int32)
    best_i2 = np.full(n1, -1, np.int64); second_i2 = np.full(n1, -1, np.int64)
    best_d = np.full(n1, MAX_HAMMING_DIST, np.int64); second_d = np.full(n1, MAX_HAMMING_DIST, np.int64); third_d = np.full(n1, MAX_HAMMING_DIST, np.int64)
    clipped = np.zeros(n1, bool)
    hist = [[] for _ in range(HIST_LEN)]            # entries (idx_1, stolen later)
    wrap_up = wrap_down = num_steals = 0
    stolen = set()
    for i1 in range(n1):
        lvl = int(kps1["octave"][i1])
        if 0 < lvl:
            reason[i1] = OCTAVE_SKIPPED
            continue
        rx, ry = pp[i1, 0], pp[i1, 1]
        lo_x = math.floor(float(f32(f32(rx - min_x) - mg)) * inv_w); hi_x = math.ceil(float(f32(f32(rx - min_x) + mg)) * inv_w)
        lo_y = math.floor(float(f32(f32(ry - min_y) - mg)) * inv_h); hi_y = math.ceil(float(f32(f32(ry - min_y) + mg)) * inv_h)
        min_cx, max_cx, min_cy, max_cy = max(0, lo_x), min(cols - 1, hi_x), max(0, lo_y), min(rows - 1, hi_y)
        if cols <= min_cx or max_cx < 0 or rows <= min_cy or max_cy < 0:
            reason[i1] = WINDOW_OUTSIDE
            continue
        clipped[i1] = lo_x < 0 or cols - 1 < hi_x or lo_y < 0 or rows - 1 < hi_y
        m = in_grid & (min_cx <= cx2) & (cx2 <= max_cx) & (min_cy <= cy2) & (cy2 <= max_cy)
        if 0 < lvl or 0 <= lvl:                      # check_level (common.cc:268): min_level = max_level = lvl; below 0 nothing is checked
            m &= (o2 >= lvl) & (o2 <= lvl)
        m &= (np.abs(x2 - rx) < mg) & (np.abs(y2 - ry) < mg)
        cand = np.nonzero(m)[0]
        if len(cand) == 0:
            continue                                  # reason stays NO_CANDIDATE
        cand = cand[np.lexsort((cand, cy2[cand], cx2[cand]))]
        best, second, third, bi, si = MAX_HAMMING_DIST, MAX_HAMMING_DIST, MAX_HAMMING_DIST, -1, -1
        for i2 in cand.tolist():
            d = int(np.unpackbits(np.bitwise_xor(d1[i1], d2[i2])).sum())
            if dists_2[i2] <= d:
                continue
            if d < best:
                third = second
                second, si = best, bi
                best, bi = d, i2
            elif d < second:
                third = second
                second, si = d, i2
            elif d < third:
                third = d
        best_i2[i1], second_i2[i1], best_d[i1], second_d[i1], third_d[i1] = bi, si, best, second, third
        if bi < 0:
            reason[i1] = ALL_HELD
            continue
        if HAMMING_DIST_THR_LOW < best:
            reason[i1] = BEST_ABOVE_50
            continue
        if f32(f32(second) * ratio) < f32(best):
            reason[i1] = RATIO_REJECTED
            continue
        prev_i1 = int(idx1_in_2[bi])
        reason[i1] = MATCHED_FRESH
        if 0 <= prev_i1:
            matched[prev_i1] = -1
            num -= 1
            stolen.add(prev_i1)
            num_steals += 1
            reason[i1] = MATCHED_STEALING
        matched[i1] = bi
        idx1_in_2[bi] = i1
        dists_2[bi] = best
        num += 1
        if check_orientation:
            b, up, down = angle_bin(kps1["angle"][i1], kps2["angle"][bi])
            hist[b].append(i1)
            wrap_up += up; wrap_down += down

    removals, bin_tie, stolen_changes = 0, False, False
    if check_orientation:
        sizes = [len(h) for h in hist]
        keep, bin_tie = valid_bins(sizes, rank_bins)
        keep_clean, _ = valid_bins([sum(i not in stolen for i in h) for h in hist], rank_bins)
        invalid = lambda kept: [i1 for b in range(HIST_LEN) if b not in kept for i1 in hist[b] if 0 <= matched[i1]]
        stolen_changes = invalid(keep) != invalid(keep_clean)     # the entry of a robbed key point stays in its bin (:123-127) and is counted
        for i1 in invalid(keep):
            matched[i1] = -1
            num -= 1
            removals += 1
    for i1 in range(n1):
        if 0 <= matched[i1]:
            pp[i1, 0] = x2[matched[i1]]; pp[i1, 1] = y2[matched[i1]]

    two = second_i2 >= 0
    facts = dict(same_lane=int((two & (best_i2 % 64 == second_i2 % 64)).sum()), different_lanes=int((two & (best_i2 % 64 != second_i2 % 64)).sum()),
                 best_equals_second=int((two & (best_d == second_d)).sum()),
                 tie_won_by_cell_order=int((two & (best_d == second_d) & (best_i2 > second_i2)).sum()),
                 orientation_removals=removals, bin_tie_at_cut=bin_tie, stolen_entry_changes_bins=stolen_changes)
    census = dict(reason=reason, best_i2=best_i2, second_i2=second_i2, best=best_d, second=second_d, third=third_d, clipped=clipped, wrap_up=int(wrap_up),
                  wrap_down=int(wrap_down), nonempty_bins=sum(1 for h in hist if h), num_steals=num_steals, facts=facts)
    return matched, pp, num, census
