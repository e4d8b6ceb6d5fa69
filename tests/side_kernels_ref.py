"""Plain numpy references of the per-frame side kernels (csrc/post_kernels.hip, the BoW transform of csrc/bow_kernels.hip) and
the small scenes both tests/test_side_kernels_cpu.py and tests/test_gpu_side_kernels.py run them on.

The references are written from the reference's sources, not from the C++ oracle (oracle/post_oracle.cpp, match_oracle.cpp):
the CPU test holds the two restatements to each other bit for bit before either judges a kernel.  Everything here is integer work
or IEEE + - * / in a fixed order, so every comparison is exact.
  to_gray            util::convert_to_grayscale   util/image_converter.cc:33-75 (cv::cvtColor on CV_8U: 14-bit fixed point)
  to_true_depth      util::convert_to_true_depth  util/image_converter.cc:77-80 (convertTo(CV_32F, 1 / factor): float scale, float work type)
  landmark_*         landmark::compute_descriptor data/landmark.cc:181-245
  color_vote         Planar_Mapping_module::create_ColorToPlane planar_mapping_module.cc:203-330, per key point
  keyline_depth      frame::compute_stereo_from_depth, key lines  data/frame.cc:1196-1217
The remap and the BoW transform keep oracle_lib's restatements (O.remap_linear, O.bow_transform).

The scenes are small on purpose: each is named for the edge it holds (a tie across the 64-row lane stride, a line whose end depth is
negative, a frame whose words all have weight zero ...), and the CPU test asserts that the edge is really there."""
import functools

import numpy as np

import oracle_lib as O

KP_DTYPE, KL_DTYPE = O.KP_DTYPE, O.KL_DTYPE


# ------------------------------------------------------------------------------------------------ references
def to_gray(src, bgr):
    """src [..., channels] u8 (3 or 4 channels; a fourth is ignored), bgr: the first channel is blue"""
    s = np.asarray(src).astype(np.int64)
    b, g, r = (s[..., 0], s[..., 1], s[..., 2]) if bgr else (s[..., 2], s[..., 1], s[..., 0])
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def to_true_depth(v, factor):
    """v u16 or f32; the scale is narrowed to float and applied in float, then + 0.0f (convertTo's shift)"""
    return (np.asarray(v).astype(np.float32) * np.float32(1.0 / factor)) + np.float32(0)


def hamming_matrix(descs):
    bits = np.unpackbits(np.ascontiguousarray(descs, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    h = bits @ (1 - bits).T                      # 0/1 products, sums <= 256: exact in f32
    return (h + h.T).astype(np.int64)


def landmark_medians(descs):
    """per row: the element of rank int(0.5 * (n - 1)) of its sorted distances to all rows, itself included"""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    n = len(d)
    return np.sort(hamming_matrix(d), axis=1)[:, int(0.5 * (n - 1))]


def landmark_descriptor(descs):
    """the first row with the smallest median; -1 for a landmark without rows"""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    if len(d) == 0:
        return -1
    return int(np.argmin(landmark_medians(d)))


def color_vote(mask, undist, valid, n, check_3x3_window):
    """mask [rows, cols, 3] u8, undist KP_DTYPE [cap], valid u8 [cap] or None, the first n key points are looked at.
    labels [cap] i32, 0 = no vote.  The `> 0` neighbour tests are the reference's: row 0 and column 0 are never looked at.  A point
    with int(y) == rows or int(x) == cols passes the reference's range test and reads outside the mask there: label 0 here."""
    rows, cols = mask.shape[:2]
    m = mask.astype(np.int64)
    lab = m[..., 0] + (m[..., 1] << 8) + (m[..., 2] << 16)
    out = np.zeros(len(undist), np.int32)
    for i in range(min(int(n), len(undist))):
        if valid is not None and not valid[i]:
            continue
        px, py = undist["x"][i], undist["y"][i]
        if py < 0 or py > np.float32(rows) or px < 0 or px > np.float32(cols):
            continue
        y, x = int(py), int(px)
        if y >= rows or x >= cols:
            continue
        center = int(lab[y, x])
        if center == 0:
            continue
        if check_3x3_window:
            colors = []
            if y + 1 > 0 and y + 1 < rows and x + 1 > 0 and x + 1 < cols: colors.append(lab[y + 1, x + 1])    # bottom right
            if y - 1 > 0 and y - 1 < rows and x - 1 > 0 and x - 1 < cols: colors.append(lab[y - 1, x - 1])    # top left
            if y + 1 > 0 and y + 1 < rows and x - 1 > 0 and x - 1 < cols: colors.append(lab[y + 1, x - 1])    # bottom left
            if y - 1 > 0 and y - 1 < rows and x + 1 > 0 and x + 1 < cols: colors.append(lab[y - 1, x + 1])    # top right
            if y + 1 > 0 and y + 1 < rows and x > 0 and x < cols: colors.append(lab[y + 1, x])                # bottom
            if y - 1 > 0 and y - 1 < rows and x > 0 and x < cols: colors.append(lab[y - 1, x])                # top
            if y > 0 and y < rows and x - 1 > 0 and x - 1 < cols: colors.append(lab[y, x - 1])                # left
            if y > 0 and y < rows and x + 1 > 0 and x + 1 < cols: colors.append(lab[y, x + 1])                # right
            if any(int(c) == 0 or int(c) != center for c in colors):
                continue
        out[i] = center
    return out


def keyline_depth(keylines, depth, fxb, kl_depths, kl_x_right):
    """keylines KL_DTYPE [n], depth [rows, cols] f32, kl_depths / kl_x_right [n, 2] pre-filled.  A line is skipped iff either end depth
    is < 0 (0 is kept: x_right = -inf); otherwise x_right = f32(f64(x) - fxb / f64(d)).  Returns the two arrays after the step."""
    kl = np.ascontiguousarray(keylines, KL_DTYPE)
    kd = np.array(kl_depths, np.float32).reshape(-1, 2); kx = np.array(kl_x_right, np.float32).reshape(-1, 2)
    sx, sy, ex, ey = kl["startPointX"], kl["startPointY"], kl["endPointX"], kl["endPointY"]
    ds = depth[sy.astype(np.int64), sx.astype(np.int64)]; de = depth[ey.astype(np.int64), ex.astype(np.int64)]     # (int) truncation
    keep = ~((ds < 0) | (de < 0))
    with np.errstate(divide="ignore"):
        xs = (sx.astype(np.float64) - np.float64(fxb) / ds.astype(np.float64)).astype(np.float32)
        xe = (ex.astype(np.float64) - np.float64(fxb) / de.astype(np.float64)).astype(np.float32)
    kd[keep, 0] = ds[keep]; kd[keep, 1] = de[keep]
    kx[keep, 0] = xs[keep]; kx[keep, 1] = xe[keep]
    return kd, kx


# ------------------------------------------------------------------------------------------------ scenes: landmark descriptor
LANDMARK_SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 1024)     # rows per landmark: around the 64-lane stride, and the header's limit
LANDMARK_SPLITS = (1, 3, 4, 5, 9)                                     # the first L of them in one call, then the rest: 1-3 idle waves in the last workgroup
LANDMARK_TIES = ("identical", "same_lane", "two_lanes", "stride", "upper_end")


def _noisy_rows(rng, n, lo, hi):
    """observations of one landmark: copies of a base row with lo .. hi - 1 bits flipped each; returns (rows, base)"""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    d = np.tile(base, (n, 1))
    for i in range(n):
        for b in rng.choice(256, int(rng.integers(lo, hi)), replace=False):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return d, base


@functools.lru_cache(maxsize=None)
def landmark_scene():
    """dict(sized=[rows of LANDMARK_SIZES], ties={name: rows}).  The ties (the census of the CPU test asserts each in the medians):
      identical  70 equal rows: every median 0, row 0 wins against every later trip and lane
      same_lane  row 70 a copy of row 6 (lane 6, second trip), the pair holds the smallest median
      two_lanes  row 37 a copy of row 5 (one trip, two lanes), the pair holds the smallest median
      stride     row 64 + 3 a copy of row 3, every other row far from all others
      upper_end  a, ~a, ~a: the median of row 0 is 256, the upper end of the kernel's search"""
    rng = np.random.default_rng(2101)
    sized = [_noisy_rows(rng, n, 0, 30)[0] for n in LANDMARK_SIZES]
    ties = {}
    ties["identical"] = np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (70, 1))
    d, base = _noisy_rows(rng, 71, 4, 30); d[6] = base; d[70] = base; ties["same_lane"] = d
    d, base = _noisy_rows(rng, 40, 4, 30); d[5] = base; d[37] = base; ties["two_lanes"] = d
    d, base = _noisy_rows(rng, 100, 60, 100); d[3] = base; d[67] = base; ties["stride"] = d
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    ties["upper_end"] = np.stack([a, ~a, ~a])
    return dict(sized=sized, ties=ties)


def pack_landmarks(rows_list):
    """-> (descs [total, 32] u8, offsets [L + 1] i32)"""
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows_list])]).astype(np.int32)
    descs = np.concatenate([np.asarray(r, np.uint8).reshape(-1, 32) for r in rows_list]) if rows_list else np.zeros((0, 32), np.uint8)
    return np.ascontiguousarray(descs), offsets


# ------------------------------------------------------------------------------------------------ scenes: key-line depth
KL_B, KL_ROWS, KL_COLS = 3, 48, 64
KL_FXB = 40.0
KL_SHAPES = ((40, 300), (300, 40), (257, 257))        # (cap, kl_cap): the grid is sized by the larger
# ragged counts per shape: over the three shapes both lists hold 0, 256, 257, cap and one value above cap (clamped to cap)
KL_COUNTS = {(40, 300): ((40, 0, 41), (257, 300, 0)), (300, 40): ((256, 257, 300), (40, 45, 0)), (257, 257): ((257, 300, 256), (256, 0, 260))}
KL_KINDS = ("positive", "zero_kept", "neg_start", "neg_end", "neg_both")
PERSPECTIVE10 = (60.0, 61.0, 31.5, 23.5, 0.1, -0.05, 0.001, -0.0007, 0.01, KL_FXB)                   # fx fy cx cy k1 k2 p1 p2 k3 fxb
FISHEYE = dict(fx=60.0, fy=60.5, cx=32.0, cy=24.0, k1=0.0035, k2=0.0007, k3=-0.002, k4=0.0002, focal_x_baseline=KL_FXB)


@functools.lru_cache(maxsize=None)
def keyline_scene(cap, kl_cap):
    """B = 3 frames of a 48 x 64 depth image, cap key points and kl_cap key lines per frame, every end point inside the image.
    Lines 0 .. 4 of every frame are the five kinds of KL_KINDS, in that order; the rest fall where they fall (5 % of the depth image
    is 0, 5 % is -1)."""
    rng = np.random.default_rng(1000 * cap + kl_cap)
    B, rows, cols = KL_B, KL_ROWS, KL_COLS
    depth = rng.uniform(0.3, 8.0, (B, rows, cols)).astype(np.float32)
    u = rng.uniform(size=depth.shape)
    depth[u < 0.05] = 0.0
    depth[u > 0.95] = -1.0
    pos1, pos2, zero, neg1, neg2 = (3, 4), (40, 60), (10, 20), (11, 21), (30, 5)      # (y, x)
    for b in range(B):
        depth[b][pos1] = 2.5; depth[b][pos2] = 1.25 + b; depth[b][zero] = 0.0; depth[b][neg1] = -1.0; depth[b][neg2] = -1.0
    kl = np.zeros((B, kl_cap), KL_DTYPE)
    for name, hi in (("startPointX", cols), ("startPointY", rows), ("endPointX", cols), ("endPointY", rows)):
        kl[name] = rng.uniform(0, hi - 0.01, (B, kl_cap)).astype(np.float32)
    for i, (s, e) in enumerate(((pos1, pos2), (zero, pos2), (neg1, pos1), (pos1, neg1), (neg1, neg2))):
        kl["startPointY"][:, i] = s[0] + 0.4; kl["startPointX"][:, i] = s[1] + 0.6
        kl["endPointY"][:, i] = e[0] + 0.9; kl["endPointX"][:, i] = e[1] + 0.1
    kl["octave"] = rng.integers(0, 3, (B, kl_cap)); kl["lineLength"] = rng.uniform(5, 60, (B, kl_cap))
    kps = np.zeros((B, cap), KP_DTYPE)
    kps["x"] = rng.uniform(0, cols - 0.01, (B, cap)); kps["y"] = rng.uniform(0, rows - 0.01, (B, cap))
    kps["size"] = 31.0; kps["angle"] = rng.uniform(0, 360, (B, cap)); kps["response"] = rng.uniform(1, 100, (B, cap))
    kps["octave"] = rng.integers(0, 8, (B, cap)); kps["class_id"] = rng.integers(0, 1000, (B, cap))
    counts, kl_counts = KL_COUNTS[(cap, kl_cap)]
    return dict(depth=depth, kl=kl, kps=kps, counts=np.array(counts, np.int32), kl_counts=np.array(kl_counts, np.int32))


def keyline_kinds(keylines, depth):
    """per line: the index into KL_KINDS"""
    kl = np.ascontiguousarray(keylines, KL_DTYPE)
    ds = depth[kl["startPointY"].astype(np.int64), kl["startPointX"].astype(np.int64)]
    de = depth[kl["endPointY"].astype(np.int64), kl["endPointX"].astype(np.int64)]
    kind = np.zeros(len(kl), np.int64)
    kind[((ds == 0) | (de == 0)) & (ds >= 0) & (de >= 0)] = 1
    kind[(ds < 0) & (de >= 0)] = 2
    kind[(ds >= 0) & (de < 0)] = 3
    kind[(ds < 0) & (de < 0)] = 4
    return kind


KL_PREFILL_DEPTH, KL_PREFILL_X_RIGHT = np.float32(-7.25), np.float32(-9.5)


@functools.lru_cache(maxsize=None)
def keyline_expected(cap, kl_cap, use_counts):
    """[B, kl_cap, 2] kl_depths and kl_x_right after the step on arrays pre-filled with KL_PREFILL_*"""
    S = keyline_scene(cap, kl_cap)
    kd = np.full((KL_B, kl_cap, 2), KL_PREFILL_DEPTH, np.float32); kx = np.full((KL_B, kl_cap, 2), KL_PREFILL_X_RIGHT, np.float32)
    for b in range(KL_B):
        n = min(int(S["kl_counts"][b]), kl_cap) if use_counts else kl_cap
        kd[b, :n], kx[b, :n] = keyline_depth(S["kl"][b, :n], S["depth"][b], KL_FXB, kd[b, :n], kx[b, :n])
    return kd, kx


# ------------------------------------------------------------------------------------------------ scenes: grey conversion, true depth
GRAY_COLS = (1, 2, 3, 4, 5, 8, 1023, 1024, 1025, 1027)      # 4 pixels per thread, 1024 per block
GRAY_ROWS, GRAY_B = 2, 2
GRAY_PLANTED = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255))


@functools.lru_cache(maxsize=None)
def gray_scene(cols, channels):
    """[B, rows, cols, channels] u8; the first pixels (as many as there are) are GRAY_PLANTED"""
    rng = np.random.default_rng(330 + 10 * cols + channels)
    src = rng.integers(0, 256, (GRAY_B, GRAY_ROWS, cols, channels), dtype=np.uint8)
    flat = src.reshape(-1, channels)
    for i, p in enumerate(GRAY_PLANTED[:len(flat)]):
        flat[i, :3] = p
    return src


DEPTH_COLS = (1, 255, 256, 257)                              # one pixel per thread, 256 per block
DEPTH_ROWS, DEPTH_B = 3, 2
DEPTH_FACTORS = (5000.0, 5208.0, 1.0, 0.001)
DEPTH_PLANTED_U16 = (0, 1, 5000, 65535)
DEPTH_PLANTED_F32_BITS = (0x80000000, 0xC0600000, 0x000116C2, 0x7F800000, 0x7FC00000)    # -0.0, -3.5, a denormal (1e-40), +inf, NaN


@functools.lru_cache(maxsize=None)
def depth_scene(cols, is_u16):
    rng = np.random.default_rng(440 + 2 * cols + int(is_u16))
    shape = (DEPTH_B, DEPTH_ROWS, cols)
    if is_u16:
        v = rng.integers(0, 65536, shape).astype(np.uint16)
        v.reshape(-1)[:len(DEPTH_PLANTED_U16)] = DEPTH_PLANTED_U16
    else:
        v = rng.uniform(-100, 40000, shape).astype(np.float32)
        v.reshape(-1).view(np.uint32)[:len(DEPTH_PLANTED_F32_BITS)] = DEPTH_PLANTED_F32_BITS
    return v


# ------------------------------------------------------------------------------------------------ scenes: colour vote
COLOR_MASKS = ((1, 1), (2, 5), (3, 3), (48, 64))
COLOR_CAPS = (255, 256, 257)
COLOR_B = 2
LABEL_A = ((10, 20, 30), (11, 20, 30))          # the frame's background label
LABEL_FOREIGN = (1, 2, 3)                       # row 0, column 0, and (2, 2) of frame 1
LABEL_C = (5, 6, 255)                           # a label whose third byte is 255


def label_of(c):
    return int(c[0]) + (int(c[1]) << 8) + (int(c[2]) << 16)


# planted key points, in this order at the front of every frame: name -> (x, y); None = depends on the mask size
COLOR_POINTS = ("x_eq_cols", "y_eq_rows", "edge_neighbours", "origin", "on_zero", "on_c", "c_border")


@functools.lru_cache(maxsize=None)
def color_scene(rows, cols, cap):
    """mask [B, rows, cols, 3], undist [B, cap], valid [B, cap] (the planted points are valid).
    Every mask: background LABEL_A[b], row 0 and column 0 LABEL_FOREIGN (masks with at least two rows and columns), pixel (2, 2) foreign
    in frame 1 only.  The 48 x 64 mask has in addition a block of label 0 and a block of LABEL_C."""
    rng = np.random.default_rng(5500 + 100 * rows + cols + cap)
    mask = np.zeros((COLOR_B, rows, cols, 3), np.uint8)
    for b in range(COLOR_B):
        mask[b] = LABEL_A[b]
        if rows >= 2 and cols >= 2:
            mask[b, 0, :] = LABEL_FOREIGN; mask[b, :, 0] = LABEL_FOREIGN
        if b == 1 and rows > 2 and cols > 2:
            mask[b, 2, 2] = LABEL_FOREIGN
        if rows >= 48 and cols >= 64:
            mask[b, 20:30, 20:40] = 0
            mask[b, 32:40, 40:60] = LABEL_C
    und = np.zeros((COLOR_B, cap), KP_DTYPE)
    und["x"] = rng.uniform(-3, cols + 3, (COLOR_B, cap)).astype(np.float32); und["y"] = rng.uniform(-3, rows + 3, (COLOR_B, cap)).astype(np.float32)
    pts = dict(x_eq_cols=(cols, min(0.5, rows - 0.5)), y_eq_rows=(min(0.5, cols - 0.5), rows), edge_neighbours=(1.3, 1.6), origin=(0.5, 0.5),
               on_zero=(25.5, 25.2), on_c=(50.2, 36.7), c_border=(40.3, 35.5))
    for i, name in enumerate(COLOR_POINTS):
        und["x"][:, i], und["y"][:, i] = pts[name]
    valid = (rng.uniform(size=(COLOR_B, cap)) > 0.1).astype(np.uint8)
    valid[:, :len(COLOR_POINTS)] = 1
    return dict(mask=mask, undist=und, valid=valid)


def color_counts(cap):
    """the count vectors a scene is run with: NULL, and ragged ones that hold 0, 256 and cap"""
    return (None, np.array([0, 256], np.int32), np.array([cap, 1], np.int32))


@functools.lru_cache(maxsize=None)
def color_expected(rows, cols, cap, use_valid, counts_idx, check):
    S = color_scene(rows, cols, cap)
    counts = color_counts(cap)[counts_idx]
    out = np.zeros((COLOR_B, cap), np.int32)
    for b in range(COLOR_B):
        n = cap if counts is None else min(int(counts[b]), cap)
        out[b] = color_vote(S["mask"][b], S["undist"][b], S["valid"][b] if use_valid else None, n, check)
    return out


# ------------------------------------------------------------------------------------------------ scenes: remap
REMAP_DCOLS = (1025, 1027)                      # 4 destination pixels per thread, 1024 per block: the second block in x runs
REMAP_DROWS, REMAP_B, REMAP_SRC = 3, 2, (33, 47)


@functools.lru_cache(maxsize=None)
def remap_scene(dcols):
    rng = np.random.default_rng(600 + dcols)
    rows, cols = REMAP_SRC
    src = rng.integers(0, 256, (REMAP_B, rows, cols), dtype=np.uint8)
    yy, xx = np.mgrid[0:REMAP_DROWS, 0:dcols].astype(np.float32)
    mx = (xx * (cols / dcols) + rng.uniform(-3, 3, xx.shape)).astype(np.float32)
    my = (yy * (rows / REMAP_DROWS) + rng.uniform(-3, 3, yy.shape)).astype(np.float32)
    mx[0, 0], my[0, 0] = -1.0, -1.0                     # just outside: only the (1, 1) tap is inside
    mx[-1, -1], my[-1, -1] = cols - 1, rows - 1         # last pixel exactly, in the second block
    mx[0, -1], my[0, -1] = 1e6, -1e6                    # far outside
    mx[-1, 0] = cols - 0.5                              # half-way into the right border
    mx[1, 1024], my[1, 1024] = 10.25, 20.75             # first pixel of the second block: known fractions
    return dict(src=src, map_x=mx, map_y=my)


# ------------------------------------------------------------------------------------------------ scenes: BoW transform
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3                    # DBoW2 WeightingType
L1_NORM, L2_NORM = 0, 1                                 # DBoW2 ScoringType (the two used here)
BOW_VOCABS = {"tfidf_l1": (10, 3, TF_IDF, L1_NORM), "tf_l2": (10, 3, TF, L2_NORM), "binary_l1": (10, 3, BINARY, L1_NORM),
              "k17_tfidf_l1": (17, 3, TF_IDF, L1_NORM)}      # k = 17: the 16-lane child loop takes two trips
BOW_CAPS = (255, 256, 257, 512, 513)                    # the LDS sort size is 256, then doubles
BOW_B = 6
BOW_LEVELSUP = 1
BOW_NONE = 0xFFFFFFFF


def bow_counts(cap):
    return np.array([cap, 0, 1, 15, 16, 17], np.int32)  # around the 16-descriptor group of the descent


def flat_tree(parents, is_leaf):
    """node list in m_nodes order -> (child_offset, children, node_word): children grouped by parent in file order, word ids handed to
    the leaves in file order (DBoW2's loaders)"""
    parents = np.asarray(parents, np.int64); is_leaf = np.asarray(is_leaf, bool)
    n = len(parents)
    children = (np.argsort(parents[1:], kind="stable") + 1).astype(np.int32)
    child_offset = np.concatenate([[0], np.cumsum(np.bincount(parents[1:], minlength=n))]).astype(np.int32)
    node_word = np.zeros(n, np.uint32)
    node_word[is_leaf] = np.arange(int(is_leaf.sum()), dtype=np.uint32)
    return child_offset, children, node_word


@functools.lru_cache(maxsize=None)
def bow_vocab(name):
    """a small random vocabulary with at least one zero-weight leaf that a descriptor can reach"""
    k, L, weighting, scoring = BOW_VOCABS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    parents, is_leaf, descs, weights = O.random_vocab(rng, k, L)
    child_offset, children, node_word = flat_tree(parents, is_leaf)
    accumulate = 1 if weighting in (TF_IDF, TF) else 0
    norm = {L1_NORM: 1, L2_NORM: 2}[scoring]
    leaves = np.flatnonzero(is_leaf)
    # where the descent takes each leaf's own descriptor (the node descriptors are random, so not always to that leaf): all weights 1
    landing = leaves[O.bow_transform(child_offset, children, descs, np.ones(len(parents)), node_word, L, descs[leaves], BOW_LEVELSUP, accumulate, norm)[0]]
    if not (weights[landing] == 0).any():
        weights = weights.copy(); weights[landing[-1]] = 0.0
    exact_zero = descs[leaves[weights[landing] == 0]]                     # descriptors that end on a zero-weight word
    exact_one = descs[leaves[np.flatnonzero(weights[landing] > 0)[0]]]    # one descriptor that ends on a word that counts
    return dict(L=L, parents=parents, is_leaf=is_leaf, descs=descs, weights=weights, weighting=weighting, scoring=scoring, child_offset=child_offset,
                children=children, node_word=node_word, accumulate=accumulate, norm=norm, leaves=leaves, exact_zero=exact_zero, exact_one=exact_one)


@functools.lru_cache(maxsize=None)
def bow_scene(name, cap):
    """desc [6, cap, 32].  Frame 0: cap copies of one leaf's descriptor (one run of cap entries owned by one thread of the assembly,
    cap - 1 sequential additions across every other thread's segment).  Frame 3: its first 15 descriptors end on zero-weight words.
    Frame 5: its first 17 descriptors are drawn from five leaves (runs that cross the 16-descriptor group)."""
    V = bow_vocab(name)
    rng = np.random.default_rng(7000 + cap + sum(map(ord, name)))
    desc = rng.integers(0, 256, (BOW_B, cap, 32), dtype=np.uint8)
    desc[0, :] = V["exact_one"]
    desc[3, :15] = V["exact_zero"][np.arange(15) % len(V["exact_zero"])]
    desc[5, :17] = V["descs"][rng.choice(V["leaves"][:5], 17)]
    return desc


@functools.lru_cache(maxsize=None)
def bow_expected(name, cap, use_counts):
    """per frame: (word_id, node_id, bow_word, bow_value, fv_node, fv_feat) of O.bow_transform on the frame's first count descriptors"""
    V = bow_vocab(name)
    desc = bow_scene(name, cap)
    counts = bow_counts(cap) if use_counts else np.full(BOW_B, cap, np.int32)
    return [O.bow_transform(V["child_offset"], V["children"], V["descs"], V["weights"], V["node_word"], V["L"], desc[b][:counts[b]], BOW_LEVELSUP,
                            V["accumulate"], V["norm"]) for b in range(BOW_B)]
