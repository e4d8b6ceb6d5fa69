"""k_match_topk_cells walks the windows of 64 queries with one lane each and stops the walk whenever one lane holds kLanePend candidate positions
or no lane has a position left; the wave then fetches the pending candidates' descriptors slot by slot (csrc/match_kernels.hip).  These cases put
the edges of that scheme into a few small frames and compare both windowed point matchers with the oracle through the entries the other matcher
tests use: a lane with more candidates than it may hold pending (the wave fetches and walks on) beside lanes with none and one, more than 16
candidates (both lists of a query overflow), waves whose candidate count is 0, exactly 64 and off 64, frames of 1 / 63 / 65 / qpb + 1 queries under
both launch shapes (32 queries per workgroup below 64 frames, 512 from 64 on), invalid and empty queries between live ones, targets beyond the
LDS hint (the walk reads them from the sorted array in memory), the stereo gate, and equal distances that the position in the key decides."""
import numpy as np
import pytest

import match_cases as MC
import oracle_lib as O
import test_gpu_match_paths as TP
from plp import plp

pytestmark = pytest.mark.gpu
SF, G64 = MC.SF8, TP.G64
CELLS_32, CELLS_512 = TP.CELLS_1, TP.CELLS_64
MODES = ["landmarks", "last_frame"]
MARGIN = {"landmarks": 12.0, "last_frame": 15.0}
PENDING_MAX = 8          # kLanePend: a query with more candidates makes its wave fetch before the lane has walked its window


def T(p, n, k):
    return p[k][:n]


def make_case(mode, probs, n, m, ints=None):
    """landmarks: levels [l - 1, l], Lowe ratio 0.8.  last frame: level_window 2 = levels [l - 1, l + 1] whatever the direction, no angle check"""
    g6, margin = O.grid6(G64), MARGIN[mode]
    if mode == "landmarks":
        def oracle(p, n, m):
            return O.match_frame_and_landmarks(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_x_right"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"),
                                               T(p, m, "q_reproj"), T(p, m, "q_x_right"), T(p, m, "q_level"), T(p, m, "q_desc"), T(p, m, "q_has_obs"), margin, 0.8)
        return TP.Case(plp.MODE_LANDMARKS, probs, n, m, oracle, ratio=0.8, ints=ints, margin=margin, scale_factors=SF, grid=G64)

    def oracle(p, n, m):
        return O.match_current_and_last(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_x_right"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"),
                                        T(p, m, "q_reproj"), T(p, m, "q_x_right"), T(p, m, "q_level"), T(p, m, "q_angle"), T(p, m, "q_desc"),
                                        T(p, m, "q_has_obs"), margin, 0, False)
    return TP.Case(plp.MODE_LAST_FRAME, probs, n, m, oracle, ratio=0.9, check=False, ints={**(ints or {}), "level_window": 2}, margin=margin,
                   scale_factors=SF, grid=G64)


def candidates(p, mode, n=None, m=None):
    """candidates per query by the rules of data::get_keypoints_in_cell for problems WITHOUT stereo coordinates: free targets inside the
    margin (strictly) on the query's levels; an invalid query has none"""
    n, m = n or len(p["t_kps"]), m or len(p["q_level"])
    kp, lvl = p["t_kps"][:n], p["q_level"][:m]
    mg = (np.float32(MARGIN[mode]) * SF[lvl])[:, None]
    dx = np.abs(kp["x"][None, :] - p["q_reproj"][:m, 0:1]); dy = np.abs(kp["y"][None, :] - p["q_reproj"][:m, 1:2])
    hi = lvl + (0 if mode == "landmarks" else 1)
    ok = (dx < mg) & (dy < mg) & (kp["octave"][None, :] >= lvl[:, None] - 1) & (kp["octave"][None, :] <= hi[:, None]) & (p["t_occupied"][:n] == 0)[None, :]
    return (ok & (p["q_valid"][:m] != 0)[:, None]).sum(1)


def empty_problem(rng, n, m):
    """n targets parked where no query looks (the image's last rows), m live queries that look at nothing (the image's first rows)"""
    kps = np.zeros(n, O.KP_DTYPE)
    kps["x"] = rng.uniform(5, 635, n).astype(np.float32); kps["y"] = rng.uniform(440, 475, n).astype(np.float32)
    kps["octave"] = 7; kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    return dict(t_kps=kps, t_desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), t_x_right=np.full(n, -1, np.float32), t_occupied=np.zeros(n, np.uint8),
                q_valid=np.ones(m, np.uint8), q_reproj=np.stack([rng.uniform(5, 635, m), rng.uniform(2, 6, m)], 1).astype(np.float32),
                q_x_right=np.full(m, -1, np.float32), q_level=np.zeros(m, np.int32), q_angle=np.full(m, 10.0, np.float32),
                q_desc=rng.integers(0, 256, (m, 32), dtype=np.uint8), q_has_obs=np.ones(m, np.uint8))


class Planter:
    """hands out target slots of a problem and the cells of a 60-pixel lattice (wider than any level-0 margin: groups do not see each other)"""

    def __init__(self, p, rng):
        self.p, self.rng, self.next_t = p, rng, 0
        self.sites = [(40.0 + 60 * i, 40.0 + 60 * j) for j in range(6) for i in range(10)]

    def group(self, queries, k):
        """k targets at graded distances 0 .. k - 1 from one descriptor, within 3 pixels of a fresh site on level 0; every query looks at them"""
        p, (x, y) = self.p, self.sites.pop(0)
        base, td = TP.graded(self.rng, k)
        t = np.arange(self.next_t, self.next_t + k); self.next_t += k
        p["t_kps"]["x"][t] = (x + self.rng.uniform(-3, 3, k)).astype(np.float32); p["t_kps"]["y"][t] = (y + self.rng.uniform(-3, 3, k)).astype(np.float32)
        p["t_kps"]["octave"][t] = 0
        p["t_desc"][t] = td
        for q in queries:
            p["q_reproj"][q] = (x, y); p["q_desc"][q] = base
        return t


# ---------------------------------------------------------------------------------------------------- per-lane overflow
@pytest.mark.parametrize("mode", MODES)
def test_a_lane_above_its_pending_capacity_and_above_both_lists(mode):
    """three frames of 70 queries.  Query 3 sees 11 targets (the wave fetches before the lane is done), queries 10, 12, .., 44 all see the same
    20 (both lists of every one of them overflow, and the 18 queries claim the 18 nearest in order: the later ones through the second
    list and the exact rescan), query 5 sees one target, the others none"""
    rng = np.random.default_rng(100 + MODES.index(mode))
    n, m, probs = 120, 70, []
    crowd_q = list(range(10, 46, 2))
    for b in range(3):
        p = empty_problem(rng, n, m)
        pl = Planter(p, rng)
        pl.group([3], 11); pl.group(crowd_q, 20); pl.group([5], 1)
        c = candidates(p, mode)
        assert PENDING_MAX < c[3] <= 16 and (c[crowd_q] == 20).all() and c[5] == 1 and c[4] == 0 and c[6] == 0 and c[64:].sum() == 0
        probs.append(p)
    case = make_case(mode, probs, n, m)
    assert TP.check_case(case, CELLS_32, 1) > 0
    if mode == "last_frame":   # no ratio test there: every query that saw a target claimed one (the landmark matcher's Lowe test rejects the near-equal ones)
        mt = plp.matcher(case.ratio, case.check)
        om, on, _ = TP.run(case, mt, "host")
        assert (on == 1 + len(crowd_q) + 1).all(), on


# ---------------------------------------------------------------------------------------------------- ragged waves
@pytest.mark.parametrize("B,plan", [(3, CELLS_32), (64, CELLS_512)], ids=["qpb32", "qpb512"])
def test_waves_with_no_pair_exactly_64_and_off_64(B, plan):
    rng = np.random.default_rng(200 + B)
    n, m, probs = 170, 192, []
    for b in range(B):
        p = empty_problem(rng, n, m)
        # 128 groups of one or two targets on a 28-pixel lattice (margin 12 on level 0: the groups do not see each other)
        sites = [(15.0 + 28 * i, 40.0 + 28 * j) for j in range(14) for i in range(22)]
        t = 0
        per_query = [2] * 32 + [1] * 32 + [0] * 64 + [2] * 5 + [1] * 27 + [1] * 27 + [0] * 5
        for q, k in enumerate(per_query):
            if not k:
                continue
            x, y = sites.pop(0)
            base, td = TP.graded(rng, k)
            for i in range(k):
                p["t_kps"]["x"][t] = x + i; p["t_kps"]["y"][t] = y; p["t_kps"]["octave"][t] = 0; p["t_desc"][t] = td[i]; t += 1
            p["q_reproj"][q] = (x, y); p["q_desc"][q] = base
        c = candidates(p, "landmarks")
        blocks = c.reshape(6, 32).sum(1)
        assert blocks.tolist() == [64, 32, 0, 0, 37, 27], blocks
        assert blocks[4] + blocks[5] == 64 and (blocks[0] + blocks[1]) % 64 != 0
        probs.append(p)
    case = make_case("landmarks", probs, n, m)
    assert case.plan() == plan
    mt = plp.matcher(case.ratio, case.check)
    res = TP.run(case, mt, "device")
    assert TP.verify(case, res, what="ragged waves") == B * int((c > 0).sum())


# ---------------------------------------------------------------------------------------------------- query counts
def dense_probs(rng, B, n, m, n_words=0, stereo=False, box=(220, 160)):
    """targets and queries inside a corner of the image: a level-0 window holds about four targets, a level-7 window dozens"""
    out = []
    for b in range(B):
        t, q = MC.random_problem(rng, n, m, n_words=n_words, cols=box[0], rows=box[1], stereo=stereo)
        out.append({**t, **q})
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,plan,n,m,counts", [(4, CELLS_32, 200, 70, [1, 63, 65, 33]), (64, CELLS_512, 40, 520, [1, 63, 65, 513])], ids=["qpb32", "qpb512"])
def test_frames_of_1_63_65_and_qpb_plus_1_queries(B, plan, n, m, counts, mode):
    rng = np.random.default_rng(300 + B + MODES.index(mode))
    case = make_case(mode, dense_probs(rng, B, n, m, n_words=6), n, m)
    assert case.plan() == plan
    qc = np.array([counts[b % 4] for b in range(B)], np.int32)
    mt = plp.matcher(case.ratio, case.check)
    assert TP.verify(case, TP.run(case, mt, "device", None, qc), None, qc, "device") > 0
    if B < 64:
        assert TP.verify(case, TP.run(case, mt, "host", None, qc), None, qc, "host") > 0


# ---------------------------------------------------------------------------------------------------- invalid and empty queries
@pytest.mark.parametrize("mode", MODES)
def test_invalid_and_empty_queries_between_live_ones(mode):
    rng = np.random.default_rng(400 + MODES.index(mode))
    n, m = 250, 140
    probs = dense_probs(rng, 3, n, m, n_words=8)
    for b, p in enumerate(probs):
        p["q_valid"][:] = 1
        p["q_valid"][b::2] = 0                                   # every other lane has no query
        p["q_reproj"][(b + 1)::3] = (-400.0, -300.0)             # every third window lies outside the grid
        p["q_reproj"][(b + 2)::7] = (630.0, 470.0)               # ... or inside it, over cells without a target
        c = candidates(p, mode)
        assert (c[b::2] == 0).all() and (c > PENDING_MAX).any() and (c == 0).sum() > m // 2
    assert TP.check_case(make_case(mode, probs, n, m), CELLS_32, 4) > 0


# ---------------------------------------------------------------------------------------------------- targets beyond the LDS hint
@pytest.mark.parametrize("mode", MODES)
def test_targets_beyond_the_lds_hint_come_from_the_sorted_array(mode):
    """t_count_hint 90 of 300 targets: the first 90 positions of the sorted array are staged, the walk and the fetch read the others from memory;
    the corner's windows straddle the boundary"""
    rng = np.random.default_rng(500 + MODES.index(mode))
    n, m = 300, 130
    case = make_case(mode, dense_probs(rng, 3, n, m, n_words=10), n, m, ints={"t_count_hint": 90})
    assert TP.check_case(case, CELLS_32, 5) > 0


# ---------------------------------------------------------------------------------------------------- stereo gate, ties
@pytest.mark.parametrize("mode", MODES)
def test_stereo_coordinates_gate_the_candidates(mode):
    rng = np.random.default_rng(600 + MODES.index(mode))
    n, m = 300, 130
    probs = dense_probs(rng, 3, n, m, n_words=10, stereo=True)
    assert all((p["t_x_right"] > 0).any() and (p["t_x_right"] <= 0).any() for p in probs)
    assert TP.check_case(make_case(mode, probs, n, m), CELLS_32, 6) > 0


@pytest.mark.parametrize("mode", MODES)
def test_equal_distances_are_decided_by_the_position(mode):
    """two descriptors in all: every window is full of candidates at the same distance, the visiting order picks among them"""
    rng = np.random.default_rng(700 + MODES.index(mode))
    n, m, probs = 260, 130, []
    for b in range(3):
        t, q = MC.random_problem(rng, n, m, n_words=2, cols=220, rows=160)
        vocab = np.unique(t["t_desc"], axis=0)[:2]
        t["t_desc"] = vocab[rng.integers(0, len(vocab), n)].copy()           # exact duplicates: no flipped bit
        q["q_desc"] = vocab[rng.integers(0, len(vocab), m)].copy()
        probs.append({**t, **q})
    assert TP.check_case(make_case(mode, probs, n, m), CELLS_32, 7) > 0
