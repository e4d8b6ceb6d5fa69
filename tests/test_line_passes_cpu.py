"""The oracle of the line front end pinned at the sweep's frame sizes (tests/line_pass_frames.py), without a GPU.

1. A plain numpy restatement in int64 -- 8.8 taps, BORDER_REFLECT_101 by index arithmetic, (sum_j k_j sum_i k_i src + 32768) >> 16,
   INTER_LINEAR_EXACT at x0.5 with half-to-even sizes, Sobel 3x3 -- must equal LineOracle's scaled plane and Sobel planes exactly: the suite
   never held the oracle to anything below 240 x 320, and the GPU sweep is only worth what the oracle is at these sizes.
2. The conditions tests/test_gpu_line_passes.py relies on: every image yields LSD segments and key lines in both seed orders (so the Sobel
   planes are compared, never skipped), and the border frames keep lines that hug the border."""
import numpy as np
import pytest

import line_pass_frames as F
import oracle_lib as O


def reflect101(p, n):
    """BORDER_REFLECT_101 of the index array p into [0, n): ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ... (period 2 n - 2)"""
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q >= n, 2 * n - 2 - q, q)


def taps(n, sigma):
    k = np.asarray(O.gaussian_taps_q8(n, sigma), np.int64)
    assert len(k) == n and np.array_equal(k, k[::-1]) and k.sum() == 256 and (k >= 0).all(), k   # (the two outer taps of the 11-tap kernel round to 0)
    return k


def blur(img, k):
    r = len(k) // 2
    h, w = img.shape
    s = img.astype(np.int64)
    hs = sum(k[i] * s[:, reflect101(np.arange(w) + i - r, w)] for i in range(len(k)))
    vs = sum(k[j] * hs[reflect101(np.arange(h) + j - r, h), :] for j in range(len(k)))
    return (vs + 32768) >> 16


def exact_coeffs(ssize, dsize):
    """first source sample and 8.8 weight of the second one per destination sample; at the borders one sample with weight 256"""
    scale = 1.0 / (dsize / ssize)
    val = (np.arange(dsize) + 0.5) * scale - 0.5
    iv = np.floor(val).astype(np.int64)
    inner = (iv >= 0) & (ssize > 1) & (iv < ssize - 1)
    o0 = np.where(iv < 0, 0, np.minimum(iv, ssize - 1))
    o1 = np.where(inner, o0 + 1, o0)
    c1 = np.where(inner, np.rint((val - iv) * 256.0), 0).astype(np.int64)
    return o0, o1, c1


def half(img):
    h, w = img.shape
    dh, dw = int(np.rint(h * 0.5)), int(np.rint(w * 0.5))       # cvRound: half to even
    assert dh in (h // 2, (h + 1) // 2) and dw in (w // 2, (w + 1) // 2)
    if h % 4 == 3: assert 2 * dh > h
    if w % 4 == 3: assert 2 * dw > w
    x0, x1, xc = exact_coeffs(w, dw)
    y0, y1, yc = exact_coeffs(h, dh)
    s = img.astype(np.int64)
    hv = s[:, x0] * (256 - xc) + s[:, x1] * xc
    v = hv[y0, :] * (256 - yc)[:, None] + hv[y1, :] * yc[:, None]
    return (v + 32768) >> 16


def sobel(img):
    h, w = img.shape
    s = img.astype(np.int64)
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    sm_y = s[ym, :] + 2 * s + s[yp, :]
    sm_x = s[:, xm] + 2 * s + s[:, xp]
    return sm_y[:, xp] - sm_y[:, xm], sm_x[yp, :] - sm_x[ym, :]


def test_reflect101_is_the_reflection():
    def by_steps(p, n):
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * (n - 1) - p
        return p
    for n in (2, 3, 16, 17):
        assert reflect101(np.arange(-3 * n, 3 * n), n).tolist() == [by_steps(p, n) for p in range(-3 * n, 3 * n)]
    assert reflect101(np.arange(-2, 3), 5).tolist() == [2, 1, 0, 1, 2] and reflect101(np.arange(3, 8), 5).tolist() == [3, 4, 3, 2, 1]


def test_the_sweep_has_the_shapes_it_names():
    shapes = F.sweep_shapes()
    assert len(shapes) == len(set(shapes)) == 127
    assert all(h >= 16 and w >= 16 for h, w in shapes)
    assert {w % 4 for w in F.WIDTHS} == {0, 1, 2, 3} and {h % 4 for h in F.HEIGHTS} == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def k11():
    return taps(11, 0.6 / 0.5)


@pytest.fixture(scope="module")
def k5():
    return taps(5, 1.0)


def check(img, k11, k5, what):
    exact, stable = O.LineOracle(img, stable_order=False), O.LineOracle(img, stable_order=True)
    for order, ora in (("libstdc++", exact), ("stable", stable)):
        assert len(ora.raw) > 0 and len(ora.all_kl) > 0, f"{what}, {order} order: {len(ora.raw)} segments, {len(ora.all_kl)} key lines"
    want = half(blur(img, k11))
    assert exact.scaled.shape == want.shape, f"{what}: half size {exact.scaled.shape}, restated {want.shape}"
    assert np.array_equal(exact.scaled, want) and np.array_equal(stable.scaled, want), f"{what}: 11-tap blur + x0.5 INTER_LINEAR_EXACT"
    dx, dy = sobel(blur(img, k5))
    assert np.array_equal(exact.dx, dx) and np.array_equal(stable.dx, dx), f"{what}: 5-tap blur + Sobel dx"
    assert np.array_equal(exact.dy, dy) and np.array_equal(stable.dy, dy), f"{what}: 5-tap blur + Sobel dy"
    return exact, stable


@pytest.mark.parametrize("part", ["widths", "heights", "tiny"])
def test_oracle_equals_the_plain_restatement(part, k11, k5):
    shapes = {"widths": F.width_shapes(), "heights": F.height_shapes(), "tiny": F.TINY}[part]
    for shape in shapes:
        for name, img in F.images(shape):
            assert img.shape == shape and img.dtype == np.uint8
            check(img, k11, k5, f"{shape} {name}")


def test_border_frames_keep_lines_that_hug_the_border(k11, k5):
    for shape, img in zip(F.BORDER_SHAPES, F.border_frames()):
        for ora in check(img, k11, k5, f"{shape} edges"):
            hug = F.border_hugging(ora.keylsd, shape)
            assert len(hug) >= 4, f"{shape}: {len(hug)} kept lines within 3 px of a border"


def test_batch_and_walk_frames_have_key_lines():
    """the other frames of the GPU file: distinct frames in every batch, key lines in every frame (the oracle's default order is the one a new context has)"""
    for shape, B in F.BATCHES + [F.UNALIGNED_BATCH]:
        frames = F.batch_frames(shape, B)
        assert frames.shape == (B,) + shape and len({f.tobytes() for f in frames}) == B
        for f in range(B):
            assert len(O.LineOracle(frames[f]).all_kl) > 0, (shape, B, f)
    assert F.WALK[0] == F.WALK[-1] and len(set(F.WALK)) == len(F.WALK) - 1
    for shape in F.WALK:
        for stable in (False, True):
            assert len(O.LineOracle(F.canvas(shape), stable_order=stable).all_kl) > 0, shape
