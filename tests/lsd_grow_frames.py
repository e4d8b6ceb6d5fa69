"""Frames for tests/test_lsd_grow_cpu.py and tests/test_gpu_lsd_grow.py: built for the branches of LSD region growing, the rectangle fits and the
refinement (k_lsd_grow / k_lsd_grow_mw), not for looking like a scene.  Everything is derived from the arguments; the two noise families draw from
named default_rng seeds.  The base size is 168 x 220 (half-resolution image 84 x 110, smallest region 12 points), so that a frame costs the oracle
well under a millisecond; the larger sizes are the ones FAMILIES names.  Which branch each family reaches is asserted on the oracle's census in
tests/test_lsd_grow_cpu.py -- that is where the parameters below were tuned."""
import functools

import numpy as np

SHAPE = (168, 220)
BIG_SHAPE = (600, 800)        # the region above 16 384 points
GRID_SHAPE = (480, 640)       # more than 2048 raw segments
BG, FG = 40, 210
NOISE_SEED, LOW_NOISE_SEED = 20261, 20262


def flat(shape=SHAPE, value=BG):
    return np.full(shape, value, np.uint8)


def _xy(shape):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return x.astype(np.float64), y.astype(np.float64)


def _blend(img, cover, value):
    """cover in [0, 1] per pixel: 1 paints `value`, between: a linear mix with what is there (soft edges give wide gradient bands)"""
    out = img.astype(np.float64) * (1.0 - cover) + value * cover
    img[...] = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return img


def bar(img, cx, cy, angle_deg, length, thick=7.0, value=FG, soft=0.0):
    """the pixels within thick / 2 of the segment of `length` px through (cx, cy) at `angle_deg`; soft > 0: the long edges fade over `soft` px"""
    x, y = _xy(img.shape)
    a = np.deg2rad(angle_deg)
    c, s = np.cos(a), np.sin(a)
    along = (x - cx) * c + (y - cy) * s
    across = -(x - cx) * s + (y - cy) * c
    inside = (np.abs(along) <= length / 2.0).astype(np.float64)
    if soft > 0:
        inside *= np.clip((thick / 2.0 - np.abs(across)) / soft + 0.5, 0.0, 1.0)
    else:
        inside *= np.abs(across) <= thick / 2.0
    return _blend(img, inside, value)


def ring(img, cx, cy, rx, ry=None, thick=5.0, a0=0.0, a1=360.0, value=FG, soft=1.0):
    """an elliptic ring (semi-axes rx, ry; ry=None: a circle) of `thick` px, between the polar angles a0 and a1 (degrees): arcs, rings, ellipses"""
    ry = rx if ry is None else ry
    x, y = _xy(img.shape)
    u, v = (x - cx) / rx, (y - cy) / ry
    r = np.sqrt(u * u + v * v)
    d = (r - 1.0) * min(rx, ry)                                  # signed distance to the centre line, exact for a circle
    cover = np.clip((thick / 2.0 - np.abs(d)) / max(soft, 1e-9) + 0.5, 0.0, 1.0)
    ang = np.rad2deg(np.arctan2(v, u)) % 360.0
    cover *= ((ang - a0) % 360.0) <= ((a1 - a0) if a1 - a0 < 360.0 else 360.0)
    return _blend(img, cover, value)


def ramp_band(img, cx, cy, angle_deg, width, length, lo=0, hi=255):
    """a band of `width` px across and `length` px along the direction `angle_deg`, whose grey level climbs linearly from lo to hi across it: one
    gradient direction over the whole band.  255 levels over 84 px are 6 levels per half-resolution pixel, just above LSD's magnitude threshold
    (2 / sin 22.5 deg = 5.23): the widest band of one direction that 8 bits can carry, 42 half-resolution pixels"""
    x, y = _xy(img.shape)
    a = np.deg2rad(angle_deg)
    c, s = np.cos(a), np.sin(a)
    along = (x - cx) * c + (y - cy) * s
    across = -(x - cx) * s + (y - cy) * c
    m = (np.abs(along) <= length / 2.0) & (np.abs(across) <= width / 2.0)
    v = lo + (hi - lo) * (across / width + 0.5)
    img[m] = np.clip(np.rint(v[m]), 0, 255).astype(np.uint8)
    return img


# ---------------------------------------------------------------------------------------------------------------- families
def bar_sweep_frames(first=24, last=215, per_frame=8, shape=SHAPE):
    """bars 5 px thick whose lengths go up in 1-px steps, eight to a frame (pitch 20 px, left-aligned at x = 2): every long edge is one region of
    about length / 2 x 2 points, the fit sizes walk through the classes <= 64, 65-128, 129-192, 193-256"""
    out, n = [], first
    while n <= last:
        img = flat(shape)
        ns = list(range(n, min(n + per_frame, last + 1)))
        for k, length in enumerate(ns):
            bar(img, 2 + length / 2.0, 12 + 20 * k, 0, length, thick=5)
        out.append((f"bars of {ns[0]}..{ns[-1]} px", img))
        n += per_frame
    return out


def wedge_frames(shape=SHAPE):
    """one edge across the frame whose blur grows along it (a step at one end, a ramp `w1` px wide at the other): the region is as wide as the edge
    is soft, so its size passes 256 by a margin that `w1` sets; straight and slanted"""
    out = []
    h, w = shape
    x, y = _xy(shape)
    for ang, w1 in ((0, 6), (0, 10), (0, 14), (0, 18), (7, 8), (7, 12), (90, 10), (83, 16)):
        a = np.deg2rad(ang)
        c, s = np.cos(a), np.sin(a)
        along = (x - w / 2.0) * c + (y - h / 2.0) * s
        across = -(x - w / 2.0) * s + (y - h / 2.0) * c
        span = float(np.abs(along).max())
        soft = 0.5 + (w1 - 0.5) * (along + span) / (2 * span)            # edge width in px at this position along the edge
        img = np.clip(np.rint(BG + (FG - BG) * np.clip(across / soft + 0.5, 0.0, 1.0)), 0, 255).astype(np.uint8)
        out.append((f"wedge at {ang} deg, edge width 0.5..{w1} px", img))
    return out


def curve_frames(shape=SHAPE):
    """rings, arcs and ellipses of radius 10-70 px and polylines with rounded corners: a region follows the curve until its angle has turned by the
    tolerance, its rectangle is mostly empty (density < 0.6), so it is regrown with the tolerance tau and shrunk pass by pass"""
    h, w = shape
    out = []
    for r in (10, 14, 19, 25, 32, 40, 50, 60, 70):
        out.append((f"ring of radius {r}", ring(flat(shape), w / 2.0 + 0.3, h / 2.0 - 0.2, r, thick=5)))
    for rx, ry in ((70, 22), (55, 35), (90, 30), (30, 64)):
        out.append((f"ellipse {rx} x {ry}", ring(flat(shape), w / 2.0, h / 2.0, rx, ry, thick=5)))
    for r, a0, a1 in ((40, 200, 340), (60, 10, 120), (70, 100, 260), (25, 300, 90)):
        out.append((f"arc of radius {r}, {a0}..{a1} deg", ring(flat(shape), w / 2.0, h / 2.0, r, thick=4, a0=a0, a1=a1)))
    for r in (6, 12, 20):     # a rounded rectangle: four bars joined by quarter rings of radius r
        img = flat(shape)
        x0, x1, y0, y1 = 40.0, w - 40.0, 30.0, h - 30.0
        bar(img, (x0 + x1) / 2, y0, 0, x1 - x0 - 2 * r, thick=4, soft=1); bar(img, (x0 + x1) / 2, y1, 0, x1 - x0 - 2 * r, thick=4, soft=1)
        bar(img, x0, (y0 + y1) / 2, 90, y1 - y0 - 2 * r, thick=4, soft=1); bar(img, x1, (y0 + y1) / 2, 90, y1 - y0 - 2 * r, thick=4, soft=1)
        for cx, cy, a0 in ((x0 + r, y0 + r, 180), (x1 - r, y0 + r, 270), (x1 - r, y1 - r, 0), (x0 + r, y1 - r, 90)):
            ring(img, cx, cy, r, thick=4, a0=a0, a1=a0 + 90)
        out.append((f"rounded rectangle, corner radius {r}", img))
    return out


def long_arc_frames(shape=SHAPE):
    """arcs of large radius with soft edges 8-12 px wide: regions above 400 points with low density, so that a shrink pass moves many points"""
    h, w = shape
    out = []
    for r, thick, soft, cy in ((150, 22, 10, 190), (200, 26, 12, 235), (120, 20, 9, 160), (260, 24, 11, 300), (170, 30, 14, 215)):
        out.append((f"long arc of radius {r}, edges {soft} px soft", ring(flat(shape), w / 2.0, float(cy), r, thick=thick, soft=soft)))
    out.append(("long arc of radius 180 from the left", ring(flat(shape), -110.0, h / 2.0, 180, thick=24, soft=11)))
    return out


def ramp_frames(shape=SHAPE):
    """bands 84 px (42 half-resolution pixels) wide with a linear ramp across: the largest regions and frontiers a frame of this size can hold"""
    h, w = shape
    out = []
    for ang in (0, 90, 45, 135, 20, 70):
        out.append((f"ramp band at {ang} deg", ramp_band(flat(shape, 128), w / 2.0, h / 2.0, ang, 84, 2 * max(h, w))))
    out.append(("two ramp bands, 0 deg", ramp_band(ramp_band(flat(shape, 128), w / 2.0, 42, 0, 84, 2 * w), w / 2.0, 126, 0, 84, 2 * w, lo=255, hi=0)))
    return out


def big_ramp_frame():
    """600 x 800: one diagonal band, 42 x ~480 half-resolution pixels: a region above 16 384 points"""
    h, w = BIG_SHAPE
    return ("600 x 800 diagonal ramp band", ramp_band(flat(BIG_SHAPE, 128), w / 2.0, h / 2.0, 36.87, 84, 2 * w))


def grating(shape, angle_deg, thick, gap, margin=0):
    """bars `thick` px wide, `gap` px apart, across the whole frame but a flat margin"""
    h, w = shape
    x, y = _xy(shape)
    a = np.deg2rad(angle_deg)
    across = -(x - w / 2.0) * np.sin(a) + (y - h / 2.0) * np.cos(a)
    img = flat(shape)
    img[(np.floor(across) % (thick + gap)) < thick] = FG
    if margin:
        img[:margin] = BG; img[-margin:] = BG; img[:, :margin] = BG; img[:, -margin:] = BG
    return img


def bricks(shape, bw, bh, shift, angle_deg=0):
    """a brick wall: rows `bh` px high of alternating bricks `bw` px long, each row moved on by `shift` px; turned by `angle_deg`"""
    h, w = shape
    x, y = _xy(shape)
    a = np.deg2rad(angle_deg)
    u = (x - w / 2.0) * np.cos(a) + (y - h / 2.0) * np.sin(a)
    v = -(x - w / 2.0) * np.sin(a) + (y - h / 2.0) * np.cos(a)
    row = np.floor(v / bh)
    img = flat(shape)
    img[((np.floor((u + row * shift) / bw) + row) % 2) == 0] = FG
    return img


def grating_frames(shape=SHAPE):
    """bars 2-4 px thick, 1-3 px apart, and two sine gratings: the regions of consecutive seeds touch one another.  The slanted ones beat against the
    half-resolution grid: their regions are sparse webs of up to 3000 points that are regrown, shrunk up to 14 times with hundreds of moves in a pass,
    or dropped when the regrowth keeps the seed alone"""
    h, w = shape
    out = []
    x, y = _xy(shape)
    for ang, thick, gap, margin in ((0, 3, 2, 8), (90, 2, 2, 8), (30, 3, 1, 8), (60, 4, 2, 8), (0, 2, 1, 8),
                                    (35, 2, 2, 0), (35, 3, 2, 0), (35, 2, 3, 0), (10, 3, 1, 0), (75, 3, 1, 0), (75, 2, 2, 0)):
        out.append((f"grating at {ang} deg, {thick} px on / {gap} px off", grating(shape, ang, thick, gap, margin)))
    # upright 4 x 2 bricks: a sparse region whose points near the seed all have the seed's angle, so that the regrowth tolerance tau is 0
    out.append(("bricks 4 x 2 px, shifted 2 px a row, upright", bricks(shape, 4, 2, 2, 90)))
    for period, ang in ((9, 15), (13, 100)):
        a = np.deg2rad(ang)
        across = -(x - w / 2.0) * np.sin(a) + (y - h / 2.0) * np.cos(a)
        out.append((f"sine grating at {ang} deg, period {period}", np.rint(125 + 100 * np.sin(2 * np.pi * across / period)).astype(np.uint8)))
    return out


def smooth_noise(shape, seed, sigma, lo=0, hi=255):
    """white noise of default_rng(seed) under a Gaussian of `sigma` px, stretched to lo..hi: blobs whose regions are sparse (several shrink passes)"""
    f = np.random.default_rng(seed).standard_normal(shape)
    t = np.arange(-(int(3 * sigma) | 1), (int(3 * sigma) | 1) + 1)
    g = np.exp(-t * t / (2 * sigma * sigma)); g /= g.sum()
    f = np.apply_along_axis(lambda r: np.convolve(r, g, mode="same"), 1, f)
    f = np.apply_along_axis(lambda r: np.convolve(r, g, mode="same"), 0, f)
    f = (f - f.min()) / (f.max() - f.min())
    return np.rint(lo + (hi - lo) * f).astype(np.uint8)


def noise_frames(shape=SHAPE):
    """uniform noise over the whole range and over a quarter of it: thousands of regions of a few points, decisions inside the angle guard band;
    smoothed noise: regions of tens of points with one to four shrink passes"""
    return [("noise, 0..255", np.random.default_rng(NOISE_SEED).integers(0, 256, shape, dtype=np.uint8)),
            ("noise, 96..159", np.random.default_rng(LOW_NOISE_SEED).integers(96, 160, shape, dtype=np.uint8)),
            ("noise, 0..255, on a ring", ring(np.random.default_rng(NOISE_SEED + 2).integers(0, 256, shape, dtype=np.uint8), 110, 84, 50, thick=6)),
            ("smooth noise, sigma 3", smooth_noise(shape, NOISE_SEED + 3, 3.0)), ("smooth noise, sigma 6", smooth_noise(shape, NOISE_SEED + 4, 6.0))]


def square_grid_frame(shape=GRID_SHAPE, side=13, pitch=18):
    """480 x 640: squares of `side` px every `pitch` px; each gives four segments: more than the 2048 raw segments a frame may hold"""
    h, w = shape
    img = flat(shape)
    for y0 in range(3, h - side - 2, pitch):
        for x0 in range(3, w - side - 2, pitch):
            img[y0:y0 + side, x0:x0 + side] = FG
    return (f"{h} x {w} grid of {side} px squares", img)


def grid_batch_frames():
    """the frames of the overflow batch: the overflowing grid in the middle, between two sparser grids of the same size that stay below 2048 segments"""
    return [square_grid_frame(side=15, pitch=36), square_grid_frame(), square_grid_frame(side=20, pitch=44)]


def border_frames(shape=SHAPE):
    """bars that end on each border and in each corner: the 3 x 3 neighbourhoods of their regions are clipped by the image"""
    h, w = shape
    out = [("0 deg through the left border", bar(flat(shape), 0, h / 2.0, 0, 160)), ("0 deg through the right border", bar(flat(shape), w - 1, h / 2.0, 0, 160)),
           ("90 deg through the top border", bar(flat(shape), w / 2.0, 0, 90, 140)), ("90 deg through the bottom border", bar(flat(shape), w / 2.0, h - 1, 90, 140)),
           ("0 deg along the top border", bar(flat(shape), w / 2.0, 1, 0, 2 * w)), ("0 deg along the bottom border", bar(flat(shape), w / 2.0, h - 2, 0, 2 * w)),
           ("90 deg along the left border", bar(flat(shape), 1, h / 2.0, 90, 2 * h)), ("90 deg along the right border", bar(flat(shape), w - 2, h / 2.0, 90, 2 * h))]
    for name, cx, cy, ang in (("top left", 0, 0, 45), ("top right", w - 1, 0, 135), ("bottom right", w - 1, h - 1, 45), ("bottom left", 0, h - 1, 135)):
        out.append((f"{ang} deg into the {name} corner", bar(flat(shape), cx, cy, ang, 150)))
        # a bar 40 px thick moved 20 px sideways: one of its long edges runs into the corner pixel itself
        nx, ny = -np.sin(np.deg2rad(ang)), np.cos(np.deg2rad(ang))
        out.append((f"an edge at {ang} deg through the {name} corner", bar(flat(shape), cx + 20 * nx, cy + 20 * ny, ang, 150, thick=40)))
    out.append(("a frame of bars on all four borders", bar(bar(bar(bar(flat(shape), w / 2.0, 0, 0, 2 * w, thick=9), w / 2.0, h - 1, 0, 2 * w, thick=9), 0, h / 2.0, 90, 2 * h, thick=9),
                                                           w - 1, h / 2.0, 90, 2 * h, thick=9)))
    return out


# full-resolution shapes whose half-resolution image has (sw - 1) * (sh - 1) % 64 = 0, 1 and 63: the last group of 64 seed positions is full, holds one, lacks one
SEED_GROUP_SHAPES = {0: (168, 130), 1: (132, 132), 63: (132, 128)}


def seed_group_frames():
    out = []
    for rem, shape in SEED_GROUP_SHAPES.items():
        h, w = shape
        img = ring(bar(flat(shape), w / 2.0, h / 2.0, 20, 100), w / 2.0, h / 2.0, 35, thick=4)
        out.append((f"{h} x {w}: seed positions % 64 = {rem}", img))
    return out


def half_size(shape):
    """(sh, sw) of the half-resolution image (cv::resize with fx = fy = 0.5 rounds)"""
    return int(np.rint(shape[0] * 0.5)), int(np.rint(shape[1] * 0.5))


FAMILY_NAMES = ("bars", "wedges", "curves", "long arcs", "ramps", "big ramp", "gratings", "noise", "square grid", "borders", "seed groups")


def families():
    """name -> [(frame name, image)]; 'big ramp' and 'square grid' hold the only frames above the base size"""
    return {"bars": bar_sweep_frames(), "wedges": wedge_frames(), "curves": curve_frames(), "long arcs": long_arc_frames(), "ramps": ramp_frames(),
            "big ramp": [big_ramp_frame()], "gratings": grating_frames(), "noise": noise_frames(), "square grid": [square_grid_frame()],
            "borders": border_frames(), "seed groups": seed_group_frames()}


@functools.lru_cache(maxsize=None)
def all_frames():
    """[(family, frame name, image)] of every family, in a fixed order; the images are shared: do not write to them"""
    out = [(fam, name, img) for fam, frames in families().items() for name, img in frames]
    for _, _, img in out:
        img.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(index, stable=True):
    """the oracle's run with its census on frame `index` of all_frames(), computed once per seed order and shared by the tests"""
    import oracle_lib as O
    return O.LineOracle(all_frames()[index][2], stable_order=stable, census=True)


# frames of the ramp and arc families at the sizes where k_lsd_grow takes 3 and 2 waves per workgroup (tests/test_gpu_lsd_grow.py derives and checks wpb)
def wpb_frames(shape, count):
    h, w = shape
    out = []
    for k in range(count):
        if k % 2 == 0:
            out.append((f"{h} x {w} ramp band {k}", ramp_band(flat(shape, 128), w / 2.0, h / 2.0, 20 + 35 * k, 84, 2 * max(h, w))))
        else:
            out.append((f"{h} x {w} arcs {k}", ring(ring(flat(shape), w / 2.0, h / 2.0, 60 + 25 * k, thick=6), w / 3.0, h / 3.0, 150 + 10 * k, thick=24, soft=11)))
    return out
