"""Hand-built scenes for area::match_in_consistent_area (plp_match_area_host, k_match_area): key points on a lattice, descriptors a base row with
exactly k flipped bits (so every Hamming distance is chosen), angles chosen per bin, frame-2 indices chosen where the lane of the kernel's
64-lane candidate stride matters.  Every scene is the smallest shape that reaches the edge it is named for, and carries `check(census, matched,
num)`: the assertions, on the census of tests/area_match_ref.py with the orientation check on, that the scene contains that edge.

scene(name) -> dict(g6, kps1, desc1, kps2, desc2, prev, margin, ratio, check[, kps3, desc3 (the chained scene's third frame)]).
A gadget is one or a few key points of frame 1 with the key points of frame 2 meant for them; gadgets lie further apart than the margin, so
they do not see each other.  Frame-2 indices nobody asked for are filled with key points parked where no window reaches."""
import functools

import numpy as np

import area_match_ref as R
import oracle_lib as O

f32 = np.float32
KP = O.KP_DTYPE
BASE = np.random.default_rng(20240607).integers(0, 256, 32, dtype=np.uint8)


def grid6(max_x, max_y, cols=64, rows=48, min_x=0.0, min_y=0.0):
    """camera::base's grid over the image bounds (camera/base.h:158-160, perspective.cc:55-56): float bounds, double inverse cell sizes"""
    return np.array([f32(min_x), f32(min_y), np.float64(cols) / np.float64(f32(max_x) - f32(min_x)), np.float64(rows) / np.float64(f32(max_y) - f32(min_y)),
                     cols, rows], np.float64)


def flip_bits(desc, bits):
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def flips(desc, k, salt):
    """desc with exactly k bits flipped, chosen by salt: Hamming distance k from desc"""
    return flip_bits(desc, np.random.default_rng(1000 + salt).choice(256, size=k, replace=False).tolist())


def slot(k):
    """lattice position k: 40 px apart, inside a 640 x 480 image"""
    return 25.0 + 40.0 * (k % 14), 25.0 + 40.0 * (k // 14)


class Builder:
    PARK = (400.0, 300.0, 116, 70)          # parking lattice of the fillers: origin, columns, rows; 2 px apart

    def __init__(self, g6=None, margin=15, ratio=0.9):
        self.g6 = grid6(640, 480) if g6 is None else g6
        self.margin, self.ratio = margin, ratio
        self.f1, self.f2 = [], {}

    def q(self, x, y, desc, angle=0.0, octave=0, prev=None):
        self.f1.append((x, y, angle, octave, np.array(desc, np.uint8), (x, y) if prev is None else prev))
        return len(self.f1) - 1

    def t(self, x, y, desc, angle=0.0, octave=0, at=None):
        if at is None:
            at = 0
            while at in self.f2:
                at += 1
        assert at not in self.f2
        self.f2[at] = (x, y, angle, octave, np.array(desc, np.uint8))
        return at

    def pair(self, k, a1, a2, dist=0):
        """one key point of frame 1 on lattice slot k with its lone partner: a match in the bin of a1 - a2"""
        x, y = slot(k)
        self.q(x, y, BASE, a1)
        return self.t(x + 1.0, y - 1.0, flips(BASE, dist, k), a2)

    def build(self, check, n2=None, **extra):
        n1 = len(self.f1)
        n2 = (max(self.f2) + 1 if self.f2 else 0) if n2 is None else n2
        assert all(i < n2 for i in self.f2)
        k1 = np.zeros(n1, KP); k2 = np.zeros(n2, KP)
        d1 = np.zeros((n1, 32), np.uint8)
        prev = np.zeros((n1, 2), f32)
        for i, (x, y, a, o, d, p) in enumerate(self.f1):
            k1[i]["x"], k1[i]["y"], k1[i]["angle"], k1[i]["octave"], k1[i]["size"] = x, y, a, o, 31.0
            d1[i] = d; prev[i] = p
        rng = np.random.default_rng(n2)
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)          # fillers: random descriptors
        j = np.arange(n2)
        x0, y0, pc, pr = self.PARK
        k2["x"] = x0 + 2.0 * (j % pc); k2["y"] = y0 + 2.0 * ((j // pc) % pr); k2["size"] = 31.0
        for i, (x, y, a, o, d) in self.f2.items():
            k2[i]["x"], k2[i]["y"], k2[i]["angle"], k2[i]["octave"] = x, y, a, o
            d2[i] = d
        if len(self.f2) < n2:           # no window reaches the parking area
            assert not ((prev[:, 0] > x0 - self.margin - 1) & (prev[:, 1] > y0 - self.margin - 1)).any()
        return dict(g6=self.g6, kps1=k1, desc1=d1, kps2=k2, desc2=d2, prev=prev, margin=self.margin, ratio=self.ratio, check=check, **extra)


# ---------------------------------------------------------------------------------------- sizes
def lattice(n1, n2, seed, margin=40):
    """n1 key points 30 px apart, n2 partners scattered over them: several candidates per window, neighbours that rob each other"""
    rng = np.random.default_rng(seed)
    b = Builder(margin=margin, ratio=0.9)
    for i in range(n1):
        desc = rng.integers(0, 256, 32, dtype=np.uint8)
        if i % 5 == 4:
            desc = flips(b.f1[i - 1][4], 3, i)                   # nearly its neighbour's descriptor: the two compete for the same partners
        b.q(15.5 + 30.0 * (i % 20), 15.5 + 30.0 * (i // 20), desc, float(rng.choice([0.0, 30.0, 60.0, 95.0, 200.0])), 1 if i % 11 == 10 else 0)
    for j in range(n2):
        i = j % n1
        x, y, a, _, desc, _ = b.f1[i]
        dx, dy = rng.uniform(-6, 6, 2)
        k = int(rng.choice([0, 5, 10, 20, 30, 45, 55]))
        b.t(float(f32(x + dx)), float(f32(y + dy)), flips(desc, k, j), float((a - rng.choice([0.0, 0.0, 0.0, 30.0, 60.0])) % 360.0), 1 if j % 13 == 12 else 0, at=j)
    level_0 = np.array([f[3] == 0 for f in b.f1])

    def check(c, matched, num):
        assert len(matched) == n1 and len(b.f2) == n2
        if n2 == 0:
            assert num == 0 and (c["reason"][level_0] == R.NO_CANDIDATE).all()
        else:
            assert num >= 1
        if n1 >= 63 and n2 >= 63:
            assert c["num_steals"] >= 1 and c["facts"]["different_lanes"] >= 1
    return b.build(check, n2=n2)


# ---------------------------------------------------------------------------------------- second best
def second_best(ib, i_s, it, accept):
    """best 40 at index ib, second 42 (rejected at ratio 0.9: 37.8 < 40) or 45 (accepted: 40.5) at i_s, third 60 at it: with the third taken for
    the second the rejected scene would be accepted (54 >= 40)"""
    b = Builder(margin=15, ratio=0.9)
    x, y = 105.5, 105.5
    d_second = 45 if accept else 42
    b.q(x, y, BASE)
    b.t(x + 3.0, y + 2.0, flips(BASE, 40, 1), at=ib)
    b.t(x - 4.0, y + 1.0, flips(BASE, d_second, 2), at=i_s)
    b.t(x + 1.0, y - 5.0, flips(BASE, 60, 3), at=it)

    def check(c, matched, num):
        assert (c["best_i2"][0], c["second_i2"][0], c["best"][0], c["second"][0], c["third"][0]) == (ib, i_s, 40, d_second, 60)
        assert not f32(f32(60) * f32(0.9)) < f32(40)
        assert c["reason"][0] == (R.MATCHED_FRESH if accept else R.RATIO_REJECTED) and matched[0] == (ib if accept else -1) and num == int(accept)
        assert c["facts"]["same_lane" if ib % 64 == i_s % 64 else "different_lanes"] == 1
    return b.build(check)


PLACEMENTS = dict(t_t64=(5, 69, 6), t64_t=(69, 5, 6), t_t1=(5, 6, 69), lane_of_three=(5, 69, 133), second_last=(130, 2, 66))


# ---------------------------------------------------------------------------------------- cell order
def cell_order():
    b = Builder(margin=15, ratio=1.0)           # ratio 1: a tie of best and second is accepted, so the winner shows
    b.q(105.0, 105.0, BASE); b.t(112.0, 105.0, flips(BASE, 20, 1), at=0); b.t(103.0, 105.0, flips(BASE, 20, 2), at=1)     # columns 11 and 10
    b.q(205.0, 105.0, BASE); b.t(205.0, 112.0, flips(BASE, 20, 3), at=2); b.t(205.0, 103.0, flips(BASE, 20, 4), at=3)     # rows 11 and 10 of column 20
    b.q(305.0, 105.0, BASE); b.t(303.0, 103.0, flips(BASE, 20, 5), at=4); b.t(306.0, 106.0, flips(BASE, 20, 6), at=5)     # one cell

    def check(c, matched, num):
        assert matched.tolist() == [1, 3, 4] and num == 3
        assert c["facts"]["best_equals_second"] == 3 and c["facts"]["tie_won_by_cell_order"] == 2
    return b.build(check)


# ---------------------------------------------------------------------------------------- steal chain
def steal_chain():
    b = Builder(margin=15, ratio=0.9)
    c_desc = flip_bits(BASE, range(20, 25))
    b.t(105.0, 105.0, BASE, at=0)                                    # t
    b.t(115.0, 105.0, flip_bits(c_desc, range(40, 48)), at=1)        # t2: 8 from C, 23 from A, 18 from B
    b.q(105.0, 105.0, flip_bits(BASE, range(0, 10)))                 # A: t at 10
    b.q(105.0, 105.0, flip_bits(BASE, range(0, 5)))                  # B: t at 5, robs A
    b.q(105.0, 105.0, c_desc)                                        # C: t at 5 is refused, takes t2
    b.q(95.0, 105.0, flip_bits(BASE, range(30, 35)))                 # D: sees t alone, at 5: does not rob

    def check(c, matched, num):
        assert c["reason"].tolist() == [R.MATCHED_FRESH, R.MATCHED_STEALING, R.MATCHED_FRESH, R.ALL_HELD]
        assert matched.tolist() == [-1, 0, 1, -1] and num == 2 and c["num_steals"] == 1
        assert (c["best"][2], c["second"][2]) == (8, 256)
    return b.build(check)


# ---------------------------------------------------------------------------------------- thresholds
def thresholds():
    b = Builder(margin=15, ratio=0.75)          # 40 * 0.75 == 30 exactly in float
    for k, dists in enumerate([(50,), (51,), (30, 40), (31, 40), (1,)]):
        x, y = slot(k)
        b.q(x, y, BASE)
        for j, d in enumerate(dists):
            b.t(x + 2.0 * j, y + 1.0, flips(BASE, d, 10 * k + j))

    def check(c, matched, num):
        assert c["reason"].tolist() == [R.MATCHED_FRESH, R.BEST_ABOVE_50, R.MATCHED_FRESH, R.RATIO_REJECTED, R.MATCHED_FRESH] and num == 3
        assert c["second"].tolist() == [256, 256, 40, 40, 256] and c["best"].tolist() == [50, 51, 30, 31, 1]
        assert f32(f32(40) * f32(0.75)) == f32(30)
    return b.build(check)


# ---------------------------------------------------------------------------------------- window
def window(L, T, Rt, Bm):
    """image bounds [L, Rt) x [T, Bm), 64 x 48 cells, margin 15"""
    b = Builder(g6=grid6(Rt, Bm, 64, 48, L, T), margin=15, ratio=0.9)
    n = [0]

    def lone(px, py, tx, ty, dist=20, bait=None):
        b.q(px, py, BASE)
        n[0] += 1
        if bait is not None:
            b.t(bait[0], bait[1], BASE)          # distance 0, but outside the image bounds: in no cell
        return b.t(tx, ty, flips(BASE, dist, n[0]))
    for px, py in ((L - 30.0, T + 100.0), (Rt + 30.0, T + 100.0), (L + 100.0, T - 30.0), (L + 100.0, Bm + 30.0)):   # 0-3: outside on each side
        b.q(px, py, BASE)
    want = [-1] * 4
    want.append(lone(L + 5.0, T + 200.0, L + 8.0, T + 200.0, bait=(L - 5.0, T + 200.0)))                           # 4-7: clipped at each border
    want.append(lone(Rt - 5.0, T + 200.0, Rt - 8.0, T + 200.0, bait=(Rt + 5.0, T + 200.0)))
    want.append(lone(L + 200.0, T + 5.0, L + 200.0, T + 8.0, bait=(L + 200.0, T - 5.0)))
    want.append(lone(L + 200.0, Bm - 5.0, L + 200.0, Bm - 8.0, bait=(L + 200.0, Bm + 5.0)))
    x, y = L + 300.0, T + 60.0
    below = lambda v: float(np.nextafter(f32(v), f32(0)))
    lone(x, y, x + 15.0, y, 0); want.append(-1)                                                                        # 8-11: |dx|, |dy| == margin
    lone(x, y + 50.0, x - 15.0, y + 50.0, 0); want.append(-1)
    lone(x, y + 100.0, x, y + 115.0, 0); want.append(-1)
    lone(x, y + 150.0, x, y + 135.0, 0); want.append(-1)
    want.append(lone(x, y + 200.0, below(x + 15.0), y + 200.0, 0))                                                     # 12-13: one float below it
    want.append(lone(x, y + 250.0, x, below(y + 265.0), 0))

    def check(c, matched, num):
        assert all(float(f32(v)) == v for v in (x, y, x + 15.0, x - 15.0, y + 115.0, y + 135.0))     # the differences are exactly the margin
        assert c["reason"].tolist() == [R.WINDOW_OUTSIDE] * 4 + [R.MATCHED_FRESH] * 4 + [R.NO_CANDIDATE] * 4 + [R.MATCHED_FRESH] * 2
        assert matched.tolist() == want and c["clipped"][4:8].all() and not c["clipped"][8:].any()
    return b.build(check)


# ---------------------------------------------------------------------------------------- octaves
def octaves():
    b = Builder(margin=15, ratio=0.9)
    x, y = slot(0); b.q(x, y, BASE, octave=1); b.t(x + 1.0, y, BASE)                                   # skipped despite a perfect partner
    x, y = slot(1); b.q(x, y, BASE)
    b.t(x + 1.0, y, BASE, octave=1); b.t(x - 1.0, y, BASE, octave=2); b.t(x, y - 2.0, BASE, octave=-1); want = b.t(x, y + 1.0, flips(BASE, 30, 1))
    x, y = slot(2); b.q(x, y, BASE); b.t(x + 1.0, y, BASE, octave=1)                                   # its only partner is not on level 0

    def check(c, matched, num):
        assert c["reason"].tolist() == [R.OCTAVE_SKIPPED, R.MATCHED_FRESH, R.NO_CANDIDATE] and matched.tolist() == [-1, want, -1]
        assert (c["best"][1], c["second"][1]) == (30, 256)
    return b.build(check)


def octaves_all_skipped():
    b = Builder(margin=15, ratio=0.9)
    for k in range(5):
        x, y = slot(k)
        b.q(x, y, BASE, octave=1 + k % 3, prev=(x + 0.5, y - 0.25)); b.t(x + 1.0, y, BASE)

    def check(c, matched, num):
        assert (c["reason"] == R.OCTAVE_SKIPPED).all() and num == 0 and (matched == -1).all()
    return b.build(check)


def octaves_negative():
    """a frame-1 octave below 0 switches get_keypoints_in_cell's level check off (common.cc:268): every level of frame 2 is a candidate"""
    b = Builder(margin=15, ratio=0.9)
    x, y = slot(0); b.q(x, y, BASE, octave=-1); want = b.t(x + 1.0, y, BASE, octave=3); b.t(x - 1.0, y, flips(BASE, 10, 1))

    def check(c, matched, num):
        assert matched.tolist() == [want] and (c["best"][0], c["second"][0]) == (0, 10)
    return b.build(check)


# ---------------------------------------------------------------------------------------- orientation
def orientation_wraps():
    b = Builder(margin=15, ratio=0.9)
    up = float(np.nextafter(f32(10.0), f32(20.0)))
    for k, (a1, a2) in enumerate([(10.0, 40.0), (10.0, 40.0), (10.0, up), (10.0, up), (360.0, 0.0), (350.0, 5.0), (45.0, 0.0), (200.0, 260.0), (5.0, 355.0)]):
        b.pair(k, a1, a2)

    def check(c, matched, num):
        assert c["wrap_up"] == 6 and c["wrap_down"] == 3          # -30 twice, -2^-20 twice (360 after the wrap, then 0), 360 itself, -60, -350
        assert R.angle_bin(10.0, up) == (0, True, True) and R.angle_bin(360.0, 0.0) == (0, False, True) and R.angle_bin(10.0, 40.0)[0] == 11
        assert c["nonempty_bins"] >= 4 and c["facts"]["orientation_removals"] >= 1
    return b.build(check)


def bins(sizes):
    """sizes: {bin: number of lone matches with an angle difference of 30 * bin}"""
    b = Builder(margin=15, ratio=0.9)
    k = 0
    for bn, cnt in sizes.items():
        for _ in range(cnt):
            b.pair(k, 30.0 * bn + 2.0, 2.0)
            k += 1
    return b


def orientation_two_bins():
    b = bins({0: 3, 4: 2})

    def check(c, matched, num):
        assert c["nonempty_bins"] == 2 and c["facts"]["orientation_removals"] == 0 and num == 5
    return b.build(check)


def orientation_tie():
    b = bins({0: 3, 1: 2, 2: 1, 3: 1})

    def check(c, matched, num):
        assert c["facts"]["bin_tie_at_cut"] and c["facts"]["orientation_removals"] == 1 and num == 6
    return b.build(check)


def orientation_stolen():
    """bins 0: 4 (two of them the robbers), 1: 3, 2: 2, 5: 1 standing + the entries of the two robbed key points, which stay: bin 5 survives with 3
    entries and bin 2 goes; counted without them, bin 2 would survive and bin 5 go"""
    b = bins({0: 2, 1: 3, 2: 2, 5: 1})
    for k in (8, 9):
        x, y = slot(k)
        b.t(x, y, BASE, 0.0)
        b.q(x, y, flip_bits(BASE, range(0, 10)), 150.0)           # takes it at 10, bin 5
        b.q(x, y, flip_bits(BASE, range(0, 5)), 0.0)              # robs it at 5, bin 0

    def check(c, matched, num):
        assert c["num_steals"] == 2 and c["facts"]["stolen_entry_changes_bins"] and c["facts"]["orientation_removals"] == 2 and num == 8
        assert not c["facts"]["bin_tie_at_cut"]
    return b.build(check)


# ---------------------------------------------------------------------------------------- chained
def chained():
    """three frames moving 8 px each, margin 10: frame 3 is found only from the positions the first call wrote into prev_matched_pts"""
    b = Builder(margin=10, ratio=0.9)
    rng = np.random.default_rng(5)
    k3 = np.zeros(12, KP); d3 = np.zeros((12, 32), np.uint8)
    for k in range(12):
        x, y = slot(k)
        desc = rng.integers(0, 256, 32, dtype=np.uint8)
        b.q(x, y, desc, 40.0)
        if k % 4 != 3:
            b.t(x + 8.0, y + 0.5, flips(desc, 3, k), 40.0)
        k3[k]["x"], k3[k]["y"], k3[k]["angle"] = x + 16.0, y + 1.0, 40.0
        d3[k] = flips(desc, 6, 100 + k)

    def check(c, matched, num):
        assert num == 9 and (matched[3::4] == -1).all()
    return b.build(check, kps3=k3, desc3=d3)


# ---------------------------------------------------------------------------------------- caps
def caps_n2_65535():
    b = Builder(margin=15, ratio=1.0)
    top = 65534
    x, y = slot(0); b.q(x, y, BASE); b.t(x + 1.0, y, flips(BASE, 10, 1), at=top); b.t(x - 1.0, y, flips(BASE, 30, 2), at=top - 64)       # one lane
    x, y = slot(1); b.q(x, y, BASE); b.t(x + 1.0, y + 1.0, flips(BASE, 20, 3), at=top - 1); b.t(x + 2.0, y + 2.0, flips(BASE, 20, 4), at=top - 2)   # one cell
    x, y = 105.0, 105.0; b.q(x, y, BASE); b.t(x + 7.0, y, flips(BASE, 20, 5), at=top - 5); b.t(x - 2.0, y, flips(BASE, 20, 6), at=top - 4)          # columns 11, 10
    x, y = slot(3); b.q(x, y, BASE); b.t(x, y + 1.0, flips(BASE, 50, 7), at=top - 6)

    def check(c, matched, num):
        assert len(b.f2) == 7 and matched.tolist() == [top, top - 2, top - 4, top - 6] and num == 4
        assert c["facts"]["same_lane"] == 1 and c["facts"]["tie_won_by_cell_order"] == 1 and c["facts"]["best_equals_second"] == 2
    return b.build(check, n2=65535)


def caps_grid_256():
    b = Builder(g6=grid6(1024, 1024, 256, 256), margin=6, ratio=1.0)
    b.q(1021.0, 1019.0, BASE); b.t(1022.0, 1021.5, flips(BASE, 20, 1), at=0); b.t(1022.0, 1018.0, flips(BASE, 20, 2), at=1)      # cells 65535 and 65534
    b.q(1019.0, 1005.0, BASE); b.t(1021.0, 1006.0, flips(BASE, 20, 3), at=2); b.t(1018.0, 1006.0, flips(BASE, 20, 4), at=3)      # cells 65531 and 65275

    def check(c, matched, num):
        assert matched.tolist() == [1, 3] and c["facts"]["tie_won_by_cell_order"] == 2
    return b.build(check)


SCENES = {}
for _n2 in (0, 1, 63, 64, 65, 128, 129):
    SCENES[f"sizes_n1_70_n2_{_n2}"] = functools.partial(lattice, 70, _n2, 100 + _n2)
for _n1 in (1, 63, 64, 65, 257):
    SCENES[f"sizes_n1_{_n1}_n2_130"] = functools.partial(lattice, _n1, 130, 200 + _n1)
for _name, _p in PLACEMENTS.items():
    SCENES[f"second_best_{_name}_rejected"] = functools.partial(second_best, *_p, False)
    SCENES[f"second_best_{_name}_accepted"] = functools.partial(second_best, *_p, True)
SCENES.update(cell_order=cell_order, steal_chain=steal_chain, thresholds=thresholds, window=functools.partial(window, 0.0, 0.0, 640.0, 480.0),
              window_offset_grid=functools.partial(window, -20.5, -10.25, 660.5, 490.25), octaves=octaves, octaves_all_skipped=octaves_all_skipped,
              octaves_negative=octaves_negative, orientation_wraps=orientation_wraps, orientation_two_bins=orientation_two_bins, orientation_tie=orientation_tie,
              orientation_stolen=orientation_stolen, chained=chained, caps_n2_65535=caps_n2_65535, caps_grid_256=caps_grid_256)
NAMES = tuple(SCENES)


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


def is_64x48(sc):
    return (int(sc["g6"][4]), int(sc["g6"][5])) == (64, 48)


def args(sc, check_orientation, frame=2, prev=None):
    """the arguments of oracle_lib.match_area / area_match_ref.match for frame 1 against frame `frame`"""
    return (sc["g6"], sc["kps1"], sc["desc1"], sc[f"kps{frame}"], sc[f"desc{frame}"], sc["prev"] if prev is None else prev, sc["margin"], sc["ratio"],
            bool(check_orientation))
