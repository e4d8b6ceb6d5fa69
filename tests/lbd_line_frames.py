"""Frames for tests/test_gpu_lbd_lines.py: bright bars (value 210, 7 px thick) on a flat background (40).  The flat background gives most of
every 63-row descriptor band zero gradients, which project to zeros of both signs; small frames (168 x 220: length filter 21 px) let lines of 22
samples and more reach the descriptor kernel.  Everything is derived from the arguments: no random numbers."""
import numpy as np

SHAPE = (168, 220)
ODD_SHAPE = (171, 221)     # width no multiple of 8, height no multiple of 4: the last tiles of the Sobel plane are partial
ANGLES = (0, 7, 45, 83, 90, 97, 135, 173)
BG, FG, THICK = 40, 210, 7


def bar(img, cx, cy, angle_deg, length, thick=THICK, value=FG):
    """paint the pixels within thick / 2 of the segment of `length` px through (cx, cy) at `angle_deg`"""
    h, w = img.shape
    a = np.deg2rad(angle_deg)
    c, s = np.cos(a), np.sin(a)
    y, x = np.mgrid[0:h, 0:w]
    along = (x - cx) * c + (y - cy) * s
    across = -(x - cx) * s + (y - cy) * c
    img[(np.abs(along) <= length / 2.0) & (np.abs(across) <= thick / 2.0)] = value
    return img


def flat(shape=SHAPE):
    return np.full(shape, BG, np.uint8)


def centred(angle_deg, length, shape=SHAPE):
    return bar(flat(shape), shape[1] // 2, shape[0] // 2, angle_deg, length)


# bar lengths of the direction sweep: chosen on the CPU so that the oracle's numOfPixels meet the census of test_directions_and_lengths
SWEEP_LENGTHS = (30, 33, 63, 64, 66, 74, 129, 138)


def sweep_frames():
    return [(a, n, centred(a, n)) for a in ANGLES for n in SWEEP_LENGTHS]


def parallel_bars(n_bars, shape=SHAPE, angle_deg=0, first=30, step=9, pitch=13):
    """n_bars parallel bars of growing length, `pitch` px apart across their direction, centred as a group"""
    img = flat(shape)
    a = np.deg2rad(angle_deg)
    nx, ny = -np.sin(a), np.cos(a)
    cx, cy = shape[1] // 2, shape[0] // 2
    for i in range(n_bars):
        d = (i - (n_bars - 1) / 2.0) * pitch
        bar(img, cx + d * nx, cy + d * ny, angle_deg, first + step * i)
    return img


def band_extent(kl):
    """per key line record: (x_min, y_min, x_max, y_max) of the four corners of its 63-row descriptor band, in f64 from the record's end points"""
    sx, sy, ex, ey = (kl[k].astype(np.float64) for k in ("sPointInOctaveX", "sPointInOctaveY", "ePointInOctaveX", "ePointInOctaveY"))
    n = kl["numOfPixels"].astype(np.float64)
    c, s = np.cos(kl["angle"].astype(np.float64)), np.sin(kl["angle"].astype(np.float64))
    mx, my, hw = (sx + ex) / 2, (sy + ey) / 2, np.floor((n - 1) / 2)
    xs = [mx + a * c - r * s for a in (-hw, n - 1 - hw) for r in (-31, 31)]
    ys = [my + a * s + r * c for a in (-hw, n - 1 - hw) for r in (-31, 31)]
    return np.min(xs, 0), np.min(ys, 0), np.max(xs, 0), np.max(ys, 0)


def edge_frames(shape=SHAPE):
    """bars whose bands leave the image: centres 6 px from each border, 45-degree bars into two opposite corners, and a horizontal and a vertical bar
    stepped pixel by pixel through the positions at which the band of one of its lines just stays inside / just leaves (names for the messages)"""
    h, w = shape
    out = [("0 deg at the top", bar(flat(shape), w // 2, 6, 0, 150)), ("0 deg at the bottom", bar(flat(shape), w // 2, h - 7, 0, 150)),
           ("90 deg at the left", bar(flat(shape), 6, h // 2, 90, 120)), ("90 deg at the right", bar(flat(shape), w - 5, h // 2, 90, 120)),
           ("45 deg into the top left corner", bar(flat(shape), 30, 30, 45, 70)), ("45 deg into the bottom right corner", bar(flat(shape), w - 31, h - 31, 45, 70))]
    for cy in range(33, 41):
        out.append((f"0 deg, band edge near the top, cy {cy}", bar(flat(shape), w // 2, cy, 0, 100)))
    for cx in range(w - 41, w - 33):
        out.append((f"90 deg, band edge near the right, cx {cx}", bar(flat(shape), cx, h // 2, 90, 100)))
    return out


def ragged_frames(shape=SHAPE):
    """a batch of unequal frames: no line, two lines, and three frames of twelve or more parallel bars of different lengths"""
    return [flat(shape), centred(0, 64, shape), parallel_bars(12, shape, 0), parallel_bars(13, shape, 90, first=28, step=8), parallel_bars(12, shape, 7, first=34, step=8, pitch=12)]


def odd_frames(shape=ODD_SHAPE):
    h, w = shape
    return [("90 deg at the right edge", bar(flat(shape), w - 6, h // 2, 90, 120)), ("0 deg at the bottom edge", bar(flat(shape), w // 2, h - 6, 0, 150)),
            ("45 deg into the bottom right corner", bar(flat(shape), w - 30, h - 30, 45, 70)), ("centred, 7 deg", centred(7, 129, shape)),
            ("twelve bars", parallel_bars(12, shape, 0))]
