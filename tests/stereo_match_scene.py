"""Built key points for match::stereo::compute: small stereo frames and lists of LEGAL key points that take every reachable decision of
stereo.cc:45-301 on purpose (tests/stereo_match_ref.py names them): equal Hamming distances, dist 74 / 75, the row band at exactly y +- 2 s,
octave +-1 against +-2, the right window off the level, the best offset on either end of the slide, negative, too large and zero disparity,
and correlations from 0 to the tens of thousands for the median.

Frames: left = columns 16 .. 16 + cols of synth.canvas(seed, rows, cols + 32); right row y = the same row shifted by d(y) px:
d(y) = 6 + round(5 sin(y / 25)) (1 .. 11), 0 in a 40-row band around the middle row, -3 in the last 30 rows.  Inside the zero band a 32-row block is
mirror-symmetric about column cx = cols // 2 in both eyes, so the SAD of an integer octave-0 key point on that axis is symmetric in the offset:
x_delta is exactly 0, the disparity exactly 0, and the 0.01 clamp fires.

A key point is legal when its octave is below the level count, x and y are at least 19 s + 1 from every border (s = the scale of its octave), and
y +- 2 s is inside the image: the reference indexes rows with .at() and the kernel does not bounds-check its patches, so assert_legal holds every
list to that."""
import functools

import numpy as np

import oracle_lib as O
from plp import synth

K_EXTRACT = 300                       # the extractors only build the pyramids for the built scenes


class Scene:
    """one stereo problem: frames, the oracle extractors that hold their pyramids, the lists and fxb / tb"""

    def __init__(self, name, left, right, levels, scale, fxb, tb, K=K_EXTRACT):
        self.name, self.left, self.right, self.levels, self.scale, self.fxb, self.tb, self.K = name, left, right, levels, scale, float(fxb), float(tb), K
        self.rows, self.cols = left.shape
        self.ol, self.orr = O.OrbOracle(K, scale, levels), O.OrbOracle(K, scale, levels)
        self.extracted = self.ol.extract(left), self.orr.extract(right)
        t = self.ol.tables()
        self.sf, self.isf = t["scale_factors"], t["inv_scale_factors"]
        self.levels_l = [self.ol.level_image(l) for l in range(levels)]
        self.levels_r = [self.orr.level_image(l) for l in range(levels)]
        self.kl = self.kr = self.dl = self.dr = None

    def set_lists(self, kl, kr, dl, dr, built=True):
        """built=False: the extractor's own key points, legal by construction (they may sit nearer a border than the built margin)"""
        self.kl, self.kr = np.ascontiguousarray(kl, O.KP_DTYPE), np.ascontiguousarray(kr, O.KP_DTYPE)
        self.dl, self.dr = np.ascontiguousarray(dl, np.uint8).reshape(-1, 32), np.ascontiguousarray(dr, np.uint8).reshape(-1, 32)
        if built:
            assert_legal(self.kl, self.sf, self.rows, self.cols); assert_legal(self.kr, self.sf, self.rows, self.cols)
        assert len(self.kl) == len(self.dl) and len(self.kr) == len(self.dr)
        return self

    def with_lists(self, kl, kr, dl, dr, built=True):
        """the same frames and pyramids under other lists"""
        import copy
        return copy.copy(self).set_lists(kl, kr, dl, dr, built)


def margin(sf, octave):
    return 19.0 * float(sf[octave]) + 1.0


def legal(x, y, octave, sf, rows, cols):
    if not 0 <= octave < len(sf):
        return False
    m, s = margin(sf, octave), float(sf[octave])
    x, y = float(np.float32(x)), float(np.float32(y))
    return m <= x <= cols - 1 - m and m <= y <= rows - 1 - m and np.floor(np.float32(y) - np.float32(2 * s)) >= 0 and np.ceil(np.float32(y) + np.float32(2 * s)) <= rows - 1


def assert_legal(kps, sf, rows, cols):
    for k in kps:
        assert legal(k["x"], k["y"], int(k["octave"]), sf, rows, cols), (k, rows, cols)


def disparity_of_row(y, rows):
    mid = rows // 2
    if y >= rows - 30:
        return -3
    if mid - 20 <= y < mid + 20:
        return 0
    return 6 + int(round(5 * np.sin(y / 25.0)))


def frames(seed, rows, cols):
    wide = synth.canvas(seed, rows, cols + 32)
    left = np.ascontiguousarray(wide[:, 16:16 + cols]); right = np.empty_like(left)
    for y in range(rows):
        d = disparity_of_row(y, rows)
        right[y] = wide[y, 16 + d:16 + d + cols]
    mid, cx = rows // 2, cols // 2
    for img in (left, right):                                   # the zero band: both eyes equal, so one mirror serves both
        img[mid - 16:mid + 16, cx - 16:cx] = img[mid - 16:mid + 16, cx + 1:cx + 17][:, ::-1]
    assert np.array_equal(left[mid - 20:mid + 20], right[mid - 20:mid + 20])
    return left, right


def keypoint(x, y, octave, sf):
    k = np.zeros((), O.KP_DTYPE)
    k["x"], k["y"], k["octave"], k["size"], k["angle"], k["response"], k["class_id"] = x, y, octave, 31.0 * float(sf[octave]), 0.0, 20.0, -1
    return k


def flip_bits(rng, desc, n):
    d = desc.copy()
    for b in rng.choice(256, n, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


X_JITTER = (0, 0, 1, -1, 3, -4, 5, -5, 6)                          # level pixels
OCTAVE_STEP = (-2, -1, 0, 0, 0, 1, 2)
BITS = (0, 0, 10, 40, 73, 74, 74, 75, 76, 120)


def built_lists(sc, seed, n_left=400, axis_points=True):
    """the recipe of the module docstring on the frames of `sc`: (kl, kr, dl, dr)"""
    rng = np.random.default_rng(seed)
    sf, rows, cols, nl = sc.sf, sc.rows, sc.cols, sc.levels
    octaves = [o for o in range(nl) if 2 * margin(sf, o) < min(rows, cols) - 1]
    assert octaves, "no level holds a legal key point"
    kl, dl, kr, dr = [], [], [], []

    def partners(k, d, n, exact=False):
        o, s_l = int(k["octave"]), float(sf[int(k["octave"])])
        for _ in range(n):
            orr = o if exact else int(np.clip(o + rng.choice(OCTAVE_STEP), 0, nl - 1))
            s = float(sf[orr])
            y_steps = (0.0, 0.0, 0.0, 0.5, -0.7, 2 * s, -2 * s, 2 * s + 1.01, -(2 * s + 1.01))
            x = np.float32(float(k["x"]) - disparity_of_row(int(k["y"]), rows) + (0 if exact else rng.choice(X_JITTER)) * s_l)
            y = np.float32(float(k["y"]) + (0.0 if exact else rng.choice(y_steps)))
            if not legal(x, y, orr, sf, rows, cols):
                continue
            desc = flip_bits(rng, d, 0 if exact else int(rng.choice(BITS)))
            for _ in range(2 if rng.uniform() < 0.2 else 1):     # an exact tie: the earlier right index must win
                kr.append(keypoint(x, y, orr, sf)); dr.append(desc)

    for _ in range(n_left):
        o = int(rng.choice(octaves))
        m = margin(sf, o)
        x, y = rng.uniform(m, cols - 1 - m), rng.uniform(m, rows - 1 - m)
        if rng.uniform() < 0.3:
            x, y = np.clip(np.rint(x), np.ceil(m), np.floor(cols - 1 - m)), np.clip(np.rint(y), np.ceil(m), np.floor(rows - 1 - m))
        if not legal(x, y, o, sf, rows, cols):
            continue
        k, d = keypoint(x, y, o, sf), rng.integers(0, 256, 32, dtype=np.uint8)
        kl.append(k); dl.append(d)
        partners(k, d, int(rng.integers(0, 4)))
    if axis_points:
        mid, cx = rows // 2, cols // 2
        for dy in (-10, -6, -2, 2, 6, 10):                          # the 11 x 11 patches and the slide stay inside the mirrored block
            k, d = keypoint(cx, mid + dy, 0, sf), rng.integers(0, 256, 32, dtype=np.uint8)
            kl.append(k); dl.append(d)
            partners(k, d, 1, exact=True)
    perm = rng.permutation(len(kr))
    return np.array(kl, O.KP_DTYPE), np.array(kr, O.KP_DTYPE)[perm], np.array(dl, np.uint8), np.array(dr, np.uint8).reshape(-1, 32)[perm]


def off_level_pairs(sc, seed, n=12):
    """left key points at octave 1 whose equal-descriptor partners at octave 0 sit so far left that the slide window of the LEFT key point's level
    starts before column 0 (needs a scale factor above 2): x_right * inv_scale[1] rounds below 10"""
    rng = np.random.default_rng(seed)
    sf = sc.sf
    assert sf[1] > 2.0
    kl, kr, dl, dr = [], [], [], []
    y0 = int(np.ceil(margin(sf, 1))) + 2
    for i in range(n):
        y = y0 + 7 * i                                              # octave-0 row bands are 5 rows: the pairs do not see each other
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        kl.append(keypoint(19.0 * float(sf[1]) + 3 + i, y, 1, sf)); dl.append(d)
        kr.append(keypoint(margin(sf, 0) + 0.5 * i, y, 0, sf)); dr.append(d)
    return np.array(kl, O.KP_DTYPE), np.array(kr, O.KP_DTYPE), np.array(dl, np.uint8), np.array(dr, np.uint8)


# name, rows, cols, levels, scale, fxb, tb
MAIN = (("160x208", 160, 208, 4, 1.2, 40.0, 1.0), ("161x211", 161, 211, 3, 1.5, 9.5, 1.0), ("200x320", 200, 320, 2, 2.0, 400.0, 1.0),
        ("120x160", 120, 160, 1, 1.2, 12.0, 1.0))
# 240x400 with three levels of 2.5 has a 38-row top level: the oracle and the reference build take it, plp_orb_extract refuses a level of 44 px or
# less, so that scene is held on the CPU only and 288x400 (a 46-row top level) stands in for it on the GPU
OFF_LEVEL = (("2.5/200x320", 200, 320, 2, 2.5, 400.0, 1.0), ("2.5/240x400", 240, 400, 3, 2.5, 400.0, 1.0), ("2.5/288x400", 288, 400, 3, 2.5, 400.0, 1.0))
GPU_REFUSED = ("2.5/240x400",)
REAL = ("identical", "noise")
NAMES = tuple(c[0] for c in MAIN + OFF_LEVEL) + REAL
GPU_NAMES = tuple(n for n in NAMES if n not in GPU_REFUSED)


@functools.lru_cache(maxsize=None)
def scene(name, seed=0):
    """the scene `name` (NAMES); seed varies the frames and lists of a built scene.  Cached: treat the result as read-only."""
    for i, (nm, rows, cols, levels, scale, fxb, tb) in enumerate(MAIN + OFF_LEVEL):
        if nm != name:
            continue
        left, right = frames(300 + 10 * i + seed, rows, cols)
        sc = Scene(name, left, right, levels, scale, fxb, tb)
        if i < len(MAIN):
            return sc.set_lists(*built_lists(sc, 400 + 10 * i + seed))
        a, b = built_lists(sc, 400 + 10 * i + seed, n_left=150), off_level_pairs(sc, 500 + i + seed)
        return sc.set_lists(*[np.concatenate([u, v]) for u, v in zip(a, b)])
    if name == "identical":                                         # the same image through both extractors, right list = left list
        img = synth.canvas(71 + seed, 160, 240)
        sc = Scene(name, img, img.copy(), 4, 1.2, 40.0, 1.0, K=400)
        (kl, dl), _ = sc.extracted
        return sc.set_lists(kl, kl, dl, dl, built=False)
    if name == "noise":                                             # uniform noise, the right eye 4 px further: level 0 correlates to 0, the resampled levels to thousands
        wide = np.random.default_rng(83 + seed).integers(0, 256, (160, 240 + 32), dtype=np.uint8)
        sc = Scene(name, np.ascontiguousarray(wide[:, 16:256]), np.ascontiguousarray(wide[:, 20:260]), 8, 1.2, 40.0, 1.0, K=1000)
        (kl, dl), (kr, dr) = sc.extracted
        return sc.set_lists(kl, kr, dl, dr, built=False)
    raise KeyError(name)


def noise_with_forced_pairs(n_pairs=40, seed=0):
    """the noise scene plus built octave-0 pairs of equal descriptors 10 px apart: their patches are unrelated noise, so the ones that pass the
    slide correlate around ten thousand"""
    sc = scene("noise", seed)
    rng = np.random.default_rng(900 + seed)
    m = margin(sc.sf, 0) + 12
    kl, kr, dl, dr = [], [], [], []
    for y in rng.choice(np.arange(int(m), int(sc.rows - 1 - m)), n_pairs, replace=False):
        x = float(np.rint(rng.uniform(m, sc.cols - 1 - m)))
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        kl.append(keypoint(x, y, 0, sc.sf)); kr.append(keypoint(x - 10, y, 0, sc.sf)); dl.append(d); dr.append(d)
    assert_legal(np.array(kl, O.KP_DTYPE), sc.sf, sc.rows, sc.cols); assert_legal(np.array(kr, O.KP_DTYPE), sc.sf, sc.rows, sc.cols)
    return sc.with_lists(np.concatenate([sc.kl, np.array(kl, O.KP_DTYPE)]), np.concatenate([sc.kr, np.array(kr, O.KP_DTYPE)]),
                         np.concatenate([sc.dl, np.array(dl, np.uint8)]), np.concatenate([sc.dr, np.array(dr, np.uint8)]), built=False)


def median_subsets(sc, corr, sizes=(1, 2, 33, 34, 16), n_other=5, seed=0):
    """left sub-lists of `sc` (the right list stays, so every left key point keeps its own result) in which exactly n key points reach the median
    step: n - 2 of distinct correlation spread over the whole range plus two more copies of the one in their middle, so that sorted[n // 2] falls
    among three equal entries; n_other key points that do not reach it are mixed in.  16 is built otherwise, to tell sorted[n // 2] from its
    neighbour: 7 correlations below a, then a ~ 1000 and b ~ 1600 as sorted[7] and sorted[8], 4 in (2 a, 2 b] and 3 above 2 b, all distinct.
    corr: the restatement's correlations of sc (-1 = not reached).  -> [(n, scene)]"""
    rng = np.random.default_rng(950 + seed)
    corr = np.asarray(corr)
    _, first = np.unique(np.where(corr > 0, corr, -1), return_index=True)
    pool = np.array([i for i in first if corr[i] > 0])                                 # one left index per distinct positive correlation, ascending
    others = np.nonzero(corr < 0)[0]
    out = []
    for n in sizes:
        if n == 1:
            pick = [pool[len(pool) // 2]]
        elif n == 2:
            pick = [pool[0], pool[-1]]
        elif n == 16:
            v = corr[pool]
            a, b = int(np.searchsorted(v, 1000)), int(np.searchsorted(v, 1600))
            below, between, above = pool[:a], pool[(v > 2 * v[a]) & (v <= 2 * v[b])], pool[v > 2 * v[b]]
            pick = list(below[np.linspace(0, len(below) - 1, 7).astype(int)]) + [pool[a], pool[b]] + list(between[:4]) + list(above[-3:])
            assert len(set(pick)) == 16
        else:
            q = n - 2
            chosen = pool[np.unique(np.linspace(0, len(pool) - 1, q).astype(int))]
            assert len(chosen) == q
            pick = list(chosen) + [chosen[q // 2]] * 2
        idx = rng.permutation(np.concatenate([np.array(pick), rng.choice(others, n_other, replace=False)]).astype(np.int64))
        out.append((n, sc.with_lists(sc.kl[idx], sc.kr, sc.dl[idx], sc.dr, built=False)))
    return out


def single_row_lists(sc, seed=0, n_right=65):
    """65 right key points in ONE row band, so the kernel's 64-lane pass over the right list wraps: left key point A has its only close partner at
    right index 64; B is equally far (2 bits) from right 0 and right 64, which the same lane sees in its first and second pass, and 0 must win;
    C matches nothing below 75.  -> (kl, kr, dl, dr, {"A": 64, "B": 0, "C": -1})"""
    rng = np.random.default_rng(970 + seed)
    y = next(r for r in range(int(margin(sc.sf, 0)) + 3, sc.rows) if disparity_of_row(r, sc.rows) >= 4)
    x0 = sc.cols // 2
    base = rng.integers(0, 256, 32, dtype=np.uint8)

    def bit(d, *bits):
        d = d.copy()
        for b in bits:
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    kr, dr = [], []
    for i in range(n_right):
        # right 0 sits on the true disparity, right 64 seven pixels further, beyond the slide: the two winners give different results
        kr.append(keypoint(x0 - disparity_of_row(y, sc.rows) - (0 if i == 0 else 7 if i == n_right - 1 else i % 3), y, 0, sc.sf))
        dr.append(bit(base, 0, 1, 2) if i == 0 else bit(base, 3) if i == n_right - 1 else flip_bits(rng, base, 30 + i % 40))
    kl = [keypoint(x0, y, 0, sc.sf) for _ in range(3)]
    dl = [base, bit(base, 0), rng.integers(0, 256, 32, dtype=np.uint8)]
    return (np.array(kl, O.KP_DTYPE), np.array(kr, O.KP_DTYPE), np.array(dl, np.uint8), np.array(dr, np.uint8)), dict(A=n_right - 1, B=0, C=-1)
