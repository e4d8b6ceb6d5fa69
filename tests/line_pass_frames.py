"""Frame sizes and images of the line front end's geometry sweep (tests/test_gpu_line_passes.py on the device, tests/test_line_passes_cpu.py for the oracle).

Every list is derived from constants of the kernels; when one of them changes, the entries named after it are the ones to revisit:

  blur tile       kBlurTW x kBlurTH = 128 x 32 outputs, staged with kBlurPad = 8 bytes to the left and right (144-byte rows), blur_tile.hpp
  inside-x path   blur_stage_inside_x is taken by a tile with tx0 >= 8 and tx0 + 136 <= w; every other tile goes through blur_prefetch /
                  blur_stage_prefetched, whose right-edge patch covers the dwords from dr0 = (w - tx0 + 8) >> 2 up to x <= w + R + 3
  rows_inside     rows are reflected only by a tile with ty0 < R or ty0 + 32 + R > h (R = 5: the 11-tap LSD blur, R = 2: the 5-tap LBD blur)
  Sobel block     kSobelTW x kSobelTH = 120 x 30 outputs from a blur tile that starts at (120 i - 4, 30 j - 1), line_kernels.hip
  half size       sw = cvRound(w / 2), half to even: w % 4 == 1 rounds down, w % 4 == 3 rounds UP (2 sw > w, other INTER_LINEAR_EXACT weights);
                  even w and even h run the fused k_blur_half (w % 4 == 2: a thread's second output pair lies past sw), every other size
                  k_blur_plane<5> + k_resize_exact
  single reflect  blur_reflect101 reflects once in straight-line code, enough for an image of at least 48 rows / columns; below, its loop runs
"""
import numpy as np

from plp import synth

# ---- widths (each at height 66; the even ones again at height 67: the same columns through k_blur_half and through k_blur_plane<5> + k_resize_exact)
WIDTHS = [
    119, 120, 121, 122, 123,                  # one Sobel block (120): the second block column holds 1..3 columns; w % 4 = 3, 0, 1, 2, 3
    127, 128, 129, 130, 131,                  # one blur tile (128): the second tile column holds 1..3 columns
    135, 136, 137,                            # tile column 0 stops needing the right-edge patch at w = 136 (dr0 reaches the 36 dwords of a staged row)
    239, 240, 241, 242, 243, 244, 245,        # two Sobel blocks (240): the third block column holds 1..5 columns; all four w % 4 classes of k_blur_half / the fallback
    251, 252, 253,                            # Sobel block column 1 (blur tile at x = 116) takes the inside-x path from w = 116 + 136 = 252
    255, 256, 257, 258, 259, 260, 261,        # two blur tiles (256): the third tile column holds 1..5 columns
    263, 264, 265,                            # blur tile column 1 (x = 128) takes the inside-x path from w = 128 + 136 = 264
    371, 372, 373,                            # Sobel block column 2 (blur tile at x = 236): inside-x from w = 372
    383, 384, 385, 387,                       # three blur tiles (384)
    391, 392, 393,                            # blur tile column 2 (x = 256): inside-x from w = 392
]
WIDTH_ROWS, WIDTH_ROWS_ODD = 66, 67

# ---- heights (each at widths 200 and 203: even -> k_blur_half on even heights, 203 = 3 (mod 4) -> the fallback with 2 sw > w)
HEIGHTS = [
    29, 30, 31, 32, 33, 34, 35,               # one Sobel block row (30) and one blur tile row (32): the second row of tiles holds 1..5 / 1..3 rows
    59, 60, 61,                               # two Sobel block rows (60)
    62, 63, 64, 65, 66, 67,                   # Sobel block row 1 (blur tile at y = 29, R = 2) stops reflecting at h = 29 + 32 + 2 = 63; two blur tile rows (64)
    68, 69, 70,                               # blur tile row 1 (y = 32, R = 5) stops reflecting at h = 32 + 32 + 5 = 69
    89, 90, 91,                               # three Sobel block rows (90)
    93, 95,                                   # Sobel block row 2 (blur tile at y = 59) stops reflecting at h = 59 + 34 = 93
    96, 97, 99,                               # three blur tile rows (96)
]
HEIGHT_COLS = (200, 203)

# ---- tiny frames: from the smallest admitted size (16 x 16) to just below and at the 48 rows / columns of the single reflection; the 11-tap tile of a
# 16 x 16 frame asks for columns up to w + 15 and rows up to 36 (several reflections), a 47-wide one for one reflection more than a 48-wide one; 17 and
# 21 round the half size down, 19, 23 and 47 up; (16, 300) and (300, 16) reflect repeatedly in one direction only
TINY = [(16, 16), (16, 17), (17, 16), (17, 19), (19, 17), (20, 21), (21, 22), (22, 47), (47, 22), (23, 23), (47, 48), (48, 47), (16, 300), (300, 16)]

# ---- frames whose lines hug the image border (the 63-row LBD band leaves the image on one side)
BORDER_SHAPES = [(480, 640), (120, 500)]


def width_shapes():
    return [(WIDTH_ROWS, w) for w in WIDTHS] + [(WIDTH_ROWS_ODD, w) for w in WIDTHS if w % 2 == 0]


def height_shapes():
    return [(h, w) for h in HEIGHTS for w in HEIGHT_COLS]


def sweep_shapes():
    """every (rows, cols) of the sweep, in the order widths, heights, tiny"""
    return width_shapes() + height_shapes() + list(TINY)


def edges(h, w, seed):
    """Straight edges everywhere the kernels treat specially: background 60, a rectangle [h//5 : h - h//6, w//6 : w - w//5] at 190, and bars
    along all four borders (top: 3 rows at 230, bottom: 2 rows at 20, left: 3 columns at 240, right: 2 columns at 10), Gaussian noise of sigma 1.5"""
    img = np.full((h, w), 60.0)
    img[h // 5:h - h // 6, w // 6:w - w // 5] = 190.0
    img[:3, :] = 230.0
    img[h - 2:, :] = 20.0
    img[:, :3] = 240.0
    img[:, w - 2:] = 10.0
    img += np.random.default_rng(seed).normal(0.0, 1.5, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def images(shape):
    """the two images of a shape: (name, frame)"""
    h, w = shape
    return [("canvas", canvas(shape)), ("edges", edges(h, w, 11 * h + w))]


# ---- batches: xcd_frame_major (xcd_map.hpp) renumbers the workgroups of a (tiles, B) grid only when tiles * B is a multiple of 8
BATCHES = [
    ((64, 131), 2),     # 2 x 2 blur tiles x 2 frames = 8: renumbered (k_blur_half); 2 x 3 Sobel blocks x 2 = 12: identity
    ((64, 131), 3),     # 12 and 18: identity
    ((64, 131), 8),     # both renumbered, every XCD takes one frame
    ((66, 244), 4),     # 2 x 3 blur tiles x 4 = 24: renumbered; 3 x 3 Sobel blocks x 4 = 36: identity
    ((66, 244), 8),
    ((67, 259), 8),     # the fallback: k_blur_plane<5> renumbered, k_resize_exact with the frame in blockIdx.z
]
UNALIGNED_BATCH = ((66, 244), 8)

# ---- one context through sizes that flip the fused / fallback switch, the row divisor, the resize tables and the buffer sizes; same frame first and last
WALK = [(66, 256), (67, 259), (16, 16), (66, 243), (480, 640), (17, 19), (66, 256)]


def batch_frames(shape, B):
    """B distinct frames: a window sliding over one canvas"""
    return synth.replay(40 + B + shape[1], B, shape[0], shape[1])


def canvas(shape):
    return synth.canvas(3 + shape[0] + shape[1], shape[0], shape[1])


def border_frames():
    return [edges(h, w, 11 * h + w) for h, w in BORDER_SHAPES]


def border_hugging(keylines, shape, dist=3.0):
    """the key lines both of whose end points lie within `dist` px of an image border"""
    h, w = shape
    def near(x, y):
        return np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y)) <= dist
    return keylines[near(keylines["startPointX"], keylines["startPointY"]) & near(keylines["endPointX"], keylines["endPointY"])]
