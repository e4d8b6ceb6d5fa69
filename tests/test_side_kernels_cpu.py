"""The numpy references of tests/side_kernels_ref.py against the C++ oracle's functions, bit for bit, on the scenes the GPU test runs
(tests/test_gpu_side_kernels.py), and the census of those scenes: each scene must really hold the edge it is named for -- the tie, the
skipped line, the zero-weight frame.  A reference that agrees on an empty case hides a failure.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import side_kernels_ref as R


# ------------------------------------------------------------------------------------------------ grey conversion, true depth
@pytest.mark.parametrize("channels", [3, 4])
def test_gray_reference_equals_the_oracle_and_the_planted_pixels_are_there(channels):
    for cols in R.GRAY_COLS:
        src = R.gray_scene(cols, channels)
        n_px = src.size // channels
        flat = src.reshape(-1, channels)[:, :3]
        for i, p in enumerate(R.GRAY_PLANTED[:n_px]):
            assert tuple(flat[i]) == p
        assert n_px >= len(R.GRAY_PLANTED) or cols < 3
        for bgr in (0, 1):
            got = R.to_gray(src, bgr)
            for b in range(R.GRAY_B):
                want = np.zeros((R.GRAY_ROWS, cols), np.uint8)
                O._call("oracle_convert_to_grayscale", [np.ascontiguousarray(src[b]), R.GRAY_ROWS, cols, channels, bgr, want])
                assert np.array_equal(got[b], want), (cols, channels, bgr, b)
    # the five planted pixels have known answers: black, white, and the three weights (4899 + 9617 + 1868 = 2^14)
    five = np.array(R.GRAY_PLANTED, np.uint8)
    assert R.to_gray(five, 0).tolist() == [0, 255, (255 * 4899 + 8192) >> 14, (255 * 9617 + 8192) >> 14, (255 * 1868 + 8192) >> 14]
    assert R.to_gray(five, 1).tolist() == [0, 255, (255 * 1868 + 8192) >> 14, (255 * 9617 + 8192) >> 14, (255 * 4899 + 8192) >> 14]


@pytest.mark.parametrize("is_u16", [1, 0])
def test_true_depth_reference_equals_the_oracle_and_the_planted_values_are_there(is_u16):
    fn = O.lib().oracle_convert_to_true_depth_u16 if is_u16 else O.lib().oracle_convert_to_true_depth_f32
    fn.restype = None
    assert np.float32(1e-40) * np.float32(1000) != 0              # denormals are not flushed in this process
    for cols in R.DEPTH_COLS:
        v = R.depth_scene(cols, is_u16)
        if is_u16:
            assert v.reshape(-1)[:4].tolist() == list(R.DEPTH_PLANTED_U16)
        else:
            f = v.reshape(-1)[:5]
            assert f.view(np.uint32).tolist() == list(R.DEPTH_PLANTED_F32_BITS)
            assert np.signbit(f[0]) and f[0] == 0 and f[1] < 0 and 0 < f[2] < np.finfo(np.float32).tiny and np.isposinf(f[3]) and np.isnan(f[4])
        for factor in R.DEPTH_FACTORS:
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                got = R.to_true_depth(v, factor)
            want = np.zeros(v.size, np.float32)
            fn(C.c_void_p(v.ctypes.data), C.c_size_t(v.size), C.c_double(factor), C.c_void_p(want.ctypes.data))
            assert np.array_equal(got.reshape(-1).view(np.uint32), want.view(np.uint32)), (cols, is_u16, factor)
            if not is_u16:
                out = got.reshape(-1)[:5]
                assert out[0] == 0 and not np.signbit(out[0])      # -0.0 * scale + 0.0f is +0.0: what the `+ 0.0f` is for
                assert out[1] < 0 and np.isposinf(out[3]) and np.isnan(out[4])
    assert R.to_true_depth(np.float32([1e-40]), 0.001)[0] > np.finfo(np.float32).tiny       # the denormal comes out normal at factor 0.001


# ------------------------------------------------------------------------------------------------ landmark descriptor
def test_landmark_reference_equals_the_oracle_and_the_ties_are_there():
    S = R.landmark_scene()
    assert [len(d) for d in S["sized"]] == list(R.LANDMARK_SIZES) and set(S["ties"]) == set(R.LANDMARK_TIES)
    for d in S["sized"] + [S["ties"][k] for k in R.LANDMARK_TIES]:
        want = O.landmark_descriptor(d) if len(d) else -1
        assert R.landmark_descriptor(d) == want, len(d)
    # even n: the lower median (rank n / 2 - 1)
    for n in (2, 4, 64, 128, 1024):
        assert int(0.5 * (n - 1)) == n // 2 - 1
    two = S["sized"][R.LANDMARK_SIZES.index(2)]
    assert R.landmark_medians(two).tolist() == [0, 0] and R.landmark_descriptor(two) == 0
    # the planted ties, in the reference's own median lists
    T = S["ties"]
    med = R.landmark_medians(T["identical"])
    assert len(med) == 70 and not med.any() and R.landmark_descriptor(T["identical"]) == 0
    for name, first, second, n in (("same_lane", 6, 70, 71), ("two_lanes", 5, 37, 40), ("stride", 3, 67, 100)):
        d = T[name]
        med = R.landmark_medians(d)
        assert len(d) == n and np.array_equal(d[first], d[second])
        assert med[first] == med[second] == med.min() and (med == med.min()).sum() == 2, name      # the pair, and only the pair, holds the smallest median
        assert R.landmark_descriptor(d) == first
        assert first % 64 != second % 64 or second >= 64                                          # two lanes, or one lane's second trip
    # 'stride': every other row is far from all others (60 .. 99 bits from the pair, more from each other): no median near the pair's
    med = R.landmark_medians(T["stride"])
    others = np.setdiff1d(np.arange(100), [3, 67])
    assert R.hamming_matrix(T["stride"])[3, others].min() >= 60 and med[others].min() >= med[3] + 20
    med = R.landmark_medians(T["upper_end"])
    assert med.tolist() == [256, 0, 0] and R.landmark_descriptor(T["upper_end"]) == 1


# ------------------------------------------------------------------------------------------------ key-line depth
@pytest.mark.parametrize("cap,kl_cap", R.KL_SHAPES)
def test_keyline_depth_reference_equals_the_oracle_and_every_kind_of_line_is_there(cap, kl_cap):
    S = R.keyline_scene(cap, kl_cap)
    kl = S["kl"]
    assert (kl["startPointX"] >= 0).all() and (kl["startPointX"] < R.KL_COLS).all() and (kl["endPointX"] >= 0).all() and (kl["endPointX"] < R.KL_COLS).all()
    assert (kl["startPointY"] >= 0).all() and (kl["startPointY"] < R.KL_ROWS).all() and (kl["endPointY"] >= 0).all() and (kl["endPointY"] < R.KL_ROWS).all()
    assert (S["kps"]["x"] >= 0).all() and (S["kps"]["x"] < R.KL_COLS).all() and (S["kps"]["y"] >= 0).all() and (S["kps"]["y"] < R.KL_ROWS).all()
    for use_counts in (True, False):
        kd, kx = R.keyline_expected(cap, kl_cap, use_counts)
        for b in range(R.KL_B):
            n = min(int(S["kl_counts"][b]), kl_cap) if use_counts else kl_cap
            pre_d = np.full((n, 2), R.KL_PREFILL_DEPTH, np.float32); pre_x = np.full((n, 2), R.KL_PREFILL_X_RIGHT, np.float32)
            want = O.post_extract(R.PERSPECTIVE10, S["kps"][b], S["depth"][b], kl[b, :n], pre_d, pre_x)
            assert np.array_equal(kd[b, :n].view(np.uint32), want["kl_depths"].reshape(n, 2).view(np.uint32)), (b, use_counts)
            assert np.array_equal(kx[b, :n].view(np.uint32), want["kl_x_right"].reshape(n, 2).view(np.uint32)), (b, use_counts)
            assert (kd[b, n:] == R.KL_PREFILL_DEPTH).all() and (kx[b, n:] == R.KL_PREFILL_X_RIGHT).all()
            if n == 0:
                continue
            # census: the five kinds, each in this frame; what each does to the outputs
            kind = R.keyline_kinds(kl[b, :n], S["depth"][b])
            assert kind[:5].tolist() == [0, 1, 2, 3, 4]
            assert all((kind == k).sum() >= 1 for k in range(5))
            assert (kd[b, :n][kind == 0] > 0).all() and np.isfinite(kx[b, :n][kind == 0]).all()
            assert np.isneginf(kx[b, :n][kind == 1]).any(axis=1).all() and (kd[b, :n][kind == 1] == 0).any(axis=1).all()
            assert (kd[b, :n][kind >= 2] == R.KL_PREFILL_DEPTH).all() and (kx[b, :n][kind >= 2] == R.KL_PREFILL_X_RIGHT).all()
    # the ragged counts, over the three shapes: 0, 256, 257, cap and a value above cap, in both lists
    counts = {(c, int(v)) for (c, k), (cs, ks) in R.KL_COUNTS.items() for v in cs}
    kl_counts = {(k, int(v)) for (c, k), (cs, ks) in R.KL_COUNTS.items() for v in ks}
    for pairs in (counts, kl_counts):
        values = {v for _, v in pairs}
        assert {0, 256, 257} <= values and any(v == c for c, v in pairs) and any(v > c for c, v in pairs)


# ------------------------------------------------------------------------------------------------ colour vote
@pytest.mark.parametrize("rows,cols", R.COLOR_MASKS)
def test_colour_vote_reference_equals_the_oracle_and_the_planted_points_are_there(rows, cols):
    A, F, Cc = [R.label_of(a) for a in R.LABEL_A], R.label_of(R.LABEL_FOREIGN), R.label_of(R.LABEL_C)
    assert Cc >> 16 == 255
    idx = {name: i for i, name in enumerate(R.COLOR_POINTS)}
    for cap in R.COLOR_CAPS:
        S = R.color_scene(rows, cols, cap)
        assert not np.isnan(S["undist"]["x"]).any() and not np.isnan(S["undist"]["y"]).any()
        for use_valid in (False, True):
            for ci, counts in enumerate(R.color_counts(cap)):
                for check in (0, 1):
                    got = R.color_expected(rows, cols, cap, use_valid, ci, check)
                    for b in range(R.COLOR_B):
                        n = cap if counts is None else min(int(counts[b]), cap)
                        want = _oracle_vote(S, b, rows, cols, cap, n, check, use_valid)
                        assert np.array_equal(got[b], want), (cap, use_valid, ci, check, b)
        # census, on the full frames (no counts, all valid)
        on, off = R.color_expected(rows, cols, cap, False, 0, 1), R.color_expected(rows, cols, cap, False, 0, 0)
        und = S["undist"]
        for b in range(R.COLOR_B):
            i = idx["x_eq_cols"]
            assert und["x"][b, i] == cols and 0 <= und["y"][b, i] <= rows and on[b, i] == 0 and off[b, i] == 0     # passes the range test, not the index test
            i = idx["y_eq_rows"]
            assert und["y"][b, i] == rows and 0 <= und["x"][b, i] <= cols and on[b, i] == 0 and off[b, i] == 0
            if rows >= 2 and cols >= 2:
                i = idx["edge_neighbours"]
                assert (int(und["y"][b, i]), int(und["x"][b, i])) == (1, 1) and R.label_of(S["mask"][b, 0, 0]) == F and R.label_of(S["mask"][b, 1, 0]) == F
                assert off[b, i] == A[b]
                if rows > 2 and cols > 2 and b == 1:
                    assert R.label_of(S["mask"][b, 2, 2]) == F and on[b, i] == 0       # a foreign label at (2, 2): rejected when the check is on
                else:
                    assert on[b, i] == A[b]                                             # foreign labels in row 0 / column 0 only: still accepted
                i = idx["origin"]
                assert off[b, i] == F and on[b, i] == 0
            if rows >= 48 and cols >= 64:
                assert on[b, idx["on_zero"]] == 0 and off[b, idx["on_zero"]] == 0 and not S["mask"][b, 25, 25].any()
                assert on[b, idx["on_c"]] == Cc and off[b, idx["on_c"]] == Cc
                assert on[b, idx["c_border"]] == 0 and off[b, idx["c_border"]] == Cc
                assert (on[b] != 0).sum() > 50 and (on[b] != off[b]).sum() > 3
        assert [c is None or sorted(c.tolist()) for c in R.color_counts(cap)] == [True, [0, 256], [1, cap]]


def _oracle_vote(S, b, rows, cols, cap, n, check, use_valid):
    fn = O.lib().oracle_color_vote
    fn.restype = None
    und, mask, valid = np.ascontiguousarray(S["undist"][b]), np.ascontiguousarray(S["mask"][b]), np.ascontiguousarray(S["valid"][b])
    want = np.zeros(cap, np.int32)
    fn(C.c_void_p(mask.ctypes.data), C.c_int(rows), C.c_int(cols), C.c_size_t(cols * 3), C.c_void_p(und.ctypes.data),
       C.c_void_p(valid.ctypes.data if use_valid else None), C.c_int(n), C.c_int(check), C.c_void_p(want.ctypes.data))
    return want


# ------------------------------------------------------------------------------------------------ remap, BoW: the scenes' census (the references are oracle_lib's)
def test_remap_scene_reaches_the_second_block():
    for dcols in R.REMAP_DCOLS:
        S = R.remap_scene(dcols)
        assert dcols > 1024 and S["map_x"].shape == (R.REMAP_DROWS, dcols) and S["src"].shape == (R.REMAP_B,) + R.REMAP_SRC
        want = O.remap_linear(S["src"][0], S["map_x"], S["map_y"])
        assert want[:, 1024:].any() and want[:, :1024].any()
        # the pixel with known fractions, first of the second block: 1/4 and 3/4 between its four taps
        s = S["src"][0].astype(np.int64)
        assert want[1, 1024] == (s[20, 10] * 24 * 8 * 32 + s[20, 11] * 8 * 8 * 32 + s[21, 10] * 24 * 24 * 32 + s[21, 11] * 8 * 24 * 32 + (1 << 14)) >> 15
        assert want[0, -1] == 0                                                          # far outside: the constant border


@pytest.mark.parametrize("name", list(R.BOW_VOCABS))
def test_bow_scene_holds_the_one_word_frame_and_the_zero_weight_frame(name):
    V = R.bow_vocab(name)
    k = R.BOW_VOCABS[name][0]
    assert np.diff(V["child_offset"]).max() == k and (V["weights"][V["is_leaf"]] == 0).any()
    for cap in R.BOW_CAPS:
        counts = R.bow_counts(cap)
        assert counts.tolist() == [cap, 0, 1, 15, 16, 17]
        E = R.bow_expected(name, cap, True)
        wid, nid, bw, bv, fn, ff = E[0]
        assert len(bw) == 1 and len(fn) == cap and len(wid) == cap and (wid == wid[0]).all() and wid[0] != R.BOW_NONE      # n_bow == 1, n_fv == cap
        wid, nid, bw, bv, fn, ff = E[3]
        assert len(wid) == 15 and len(bw) == 0 and len(fn) == 0 and (wid == R.BOW_NONE).all() and (nid == R.BOW_NONE).all()   # n_bow == n_fv == 0
        assert len(E[1][0]) == 0 and len(E[1][2]) == 0
        wid = E[5][0]
        assert len(wid) == 17 and len(np.unique(wid)) < 17                                                                    # repeated words in a short frame
        full = R.bow_expected(name, cap, False)
        assert all(len(f[0]) == cap for f in full) and len(full[0][2]) == 1
