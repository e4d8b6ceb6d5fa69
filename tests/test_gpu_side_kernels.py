"""The per-frame side kernels (csrc/post_kernels.hip: key-line depth, landmark descriptor, grey conversion, true depth, colour vote,
remap; csrc/bow_kernels.hip: the BoW transform) at block, stride and ragged-count edges, bit for bit against the numpy references of
tests/side_kernels_ref.py (remap and BoW: oracle_lib's).  The C entries are called directly: padded steps, frame strides with gaps,
misaligned bases, NULL optionals.  Every output buffer is filled with a sentinel and is longer than the call needs; it is compared
whole, so slots above a count, row padding, gaps between frames and the tail must come back untouched.
tests/test_side_kernels_cpu.py holds the references to the C++ oracle and asserts that each scene contains the edge it is named for."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import side_kernels_ref as R
from plp import plp

pytestmark = pytest.mark.gpu

SENT = 0xA5           # every byte of an output buffer before the call


def dev():
    import torch
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def matcher():
    return plp.matcher()          # one context for the whole file


def handle():
    return matcher()._h


def up(a):
    """host array -> device bytes (a torch tensor; .data_ptr() is NULL for an empty one)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(dev())


def down(t, dtype=np.uint8):
    return t.cpu().numpy().view(dtype)


def sync():
    import torch
    torch.cuda.synchronize()


def filled(n_bytes):
    return np.full(n_bytes, SENT, np.uint8)


def lay(dense, step, frame_stride, offset=0, tail=16, rng=None):
    """dense [B, rows, ...] -> flat bytes with row y of frame b at offset + b * frame_stride + y * step; everything else is the sentinel
    (an output's expected image) or, with rng, random bytes (an input: whatever is read outside a row shows in the result)"""
    dense = np.ascontiguousarray(dense)
    B, rows = dense.shape[:2]
    d = dense.reshape(B, rows, -1).view(np.uint8)
    rb = d.shape[2]
    assert step >= rb and frame_stride >= rows * step
    n = offset + B * frame_stride + tail
    buf = rng.integers(0, 256, n, dtype=np.uint8) if rng is not None else filled(n)
    for b in range(B):
        for y in range(rows):
            o = offset + b * frame_stride + y * step
            buf[o:o + rb] = d[b, y]
    return buf


def put(buf, dtype, at, values):
    """write `values` into the byte buffer at element index `at` of its view as dtype"""
    v = np.ascontiguousarray(values, dtype).reshape(-1)
    buf.view(dtype)[at:at + len(v)] = v


def same(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    assert len(got) == len(want), what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} bytes differ, first at {bad[:8].tolist()}: got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


# ------------------------------------------------------------------------------------------------ a. landmark descriptor
@functools.lru_cache(maxsize=None)
def landmark_cases():
    S = R.landmark_scene()
    rows = list(S["sized"]) + [S["ties"][k] for k in R.LANDMARK_TIES]
    return rows, [R.landmark_descriptor(d) for d in rows]


def check_landmarks(index):
    """the landmarks `index` of landmark_cases() in one call: the device entry on the caller's stream, then the host entry"""
    import torch
    rows, best = landmark_cases()
    descs, offsets = R.pack_landmarks([rows[i] for i in index])
    want = np.array([best[i] for i in index] + [-77] * 4, np.int32)
    L = len(index)
    mt = matcher()
    st = torch.cuda.Stream(device=dev())
    d_descs, d_off, d_best = up(descs), up(offsets), up(np.full(L + 4, -77, np.int32))
    sync()
    plp._check(plp.lib().plp_landmark_descriptor_device(mt._h, d_descs.data_ptr() or None, d_off.data_ptr(), L, d_best.data_ptr(), st.cuda_stream))
    st.synchronize()
    assert down(d_best, np.int32).tolist() == want.tolist(), ("device", index)
    h_best = np.full(L + 4, -77, np.int32)
    plp._check(plp.lib().plp_landmark_descriptor_host(mt._h, plp._p(descs) if len(descs) else None, plp._p(offsets), L, plp._p(h_best)))
    assert h_best.tolist() == want.tolist(), ("host", index)


def test_landmark_descriptor_every_size_and_planted_tie_in_one_call():
    rows, best = landmark_cases()
    n_sized = len(R.LANDMARK_SIZES)
    assert [len(d) for d in rows[:n_sized]] == list(R.LANDMARK_SIZES) and len(rows) % 4 == 1       # 17 landmarks: three idle waves in the last workgroup
    ties = dict(zip(R.LANDMARK_TIES, best[n_sized:]))
    assert ties == dict(identical=0, same_lane=6, two_lanes=5, stride=3, upper_end=1) and best[0] == -1
    check_landmarks(tuple(range(len(rows))))
    check_landmarks(tuple(range(n_sized, len(rows))))                                              # the ties alone: 5 landmarks


@pytest.mark.parametrize("L", R.LANDMARK_SPLITS)
def test_landmark_descriptor_idle_waves_in_the_last_workgroup(L):
    n_sized = len(R.LANDMARK_SIZES)
    check_landmarks(tuple(range(L)))                    # the first L sizes ...
    check_landmarks(tuple(range(L, n_sized)))           # ... then the rest


def test_landmark_descriptor_host_entry_refuses_1025_rows_and_descending_offsets():
    rng = np.random.default_rng(9)
    mt = matcher()
    descs = rng.integers(0, 256, (1030, 32), dtype=np.uint8)
    for offsets in ([0, 2, 1027, 1030], [0, 1025], [0, 5, 3, 9], [4, 0]):
        off = np.array(offsets, np.int32)
        best = np.full(len(off) + 3, -77, np.int32)
        assert plp.lib().plp_landmark_descriptor_host(mt._h, plp._p(descs), plp._p(off), len(off) - 1, plp._p(best)) == plp.PLP_ERR_UNSUPPORTED, offsets
        assert (best == -77).all(), offsets
    # exactly 1024 rows is inside the limit
    off = np.array([0, 1024, 1030], np.int32)
    best = np.full(6, -77, np.int32)
    plp._check(plp.lib().plp_landmark_descriptor_host(mt._h, plp._p(descs), plp._p(off), 2, plp._p(best)))
    assert best.tolist() == [R.landmark_descriptor(descs[:1024]), R.landmark_descriptor(descs[1024:]), -77, -77, -77, -77]


# ------------------------------------------------------------------------------------------------ b. key-line depth, batched device entries
KL_STEP = R.KL_COLS * 4 + 16
KL_FRAME_STRIDE = R.KL_ROWS * KL_STEP + 32
KP_OUTPUTS = (("undist", 28), ("bearings", 24), ("x_right", 4), ("depths", 4))     # name, bytes per key point


def perspective_camera():
    c = plp.camera_c()
    for name, v in zip(("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "focal_x_baseline"), R.PERSPECTIVE10):
        setattr(c, name, float(v))
    return c


def model_camera(model):
    c = plp.camera_model_c()
    c.model, c.cols, c.rows = model, R.KL_COLS, R.KL_ROWS
    if model == plp.CAMERA_FISHEYE:
        for name, v in R.FISHEYE.items():
            setattr(c, name, float(v))
    elif model == plp.CAMERA_PERSPECTIVE:
        for name, v in zip(("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "focal_x_baseline"), R.PERSPECTIVE10):
            setattr(c, name, float(v))
    return c


POST_ENTRIES = {"plain": ("plp_post_extract_device", perspective_camera),
                "model_perspective": ("plp_post_extract_model_device", lambda: model_camera(plp.CAMERA_PERSPECTIVE)),
                "model_fisheye": ("plp_post_extract_model_device", lambda: model_camera(plp.CAMERA_FISHEYE))}


def kl_prefilled(kl_cap):
    """the two key-line outputs before the call, as bytes: [B, kl_cap, 2] + 8 floats of tail"""
    n = R.KL_B * kl_cap * 2 + 8
    return np.full(n, R.KL_PREFILL_DEPTH, np.float32).view(np.uint8), np.full(n, R.KL_PREFILL_X_RIGHT, np.float32).view(np.uint8)


def run_post_extract(entry, camera, cap, kl_cap, use_counts, with_kps, with_kl, with_depth=True):
    """one batched call; returns (status, {output: bytes after the call})"""
    S = R.keyline_scene(cap, kl_cap)
    B = R.KL_B
    rng = np.random.default_rng(5)
    d_depth = up(lay(S["depth"], KL_STEP, KL_FRAME_STRIDE, rng=rng))
    d_kps, d_kl = up(S["kps"]), up(S["kl"])
    d_cnt, d_klcnt = up(S["counts"]), up(S["kl_counts"])
    out = {name: up(filled(B * cap * es + 2 * es)) for name, es in KP_OUTPUTS}
    pre_d, pre_x = kl_prefilled(kl_cap)
    out["kl_depths"], out["kl_x_right"] = up(pre_d), up(pre_x)
    P = lambda t, on=True: t.data_ptr() if on else None
    sync()
    status = getattr(plp.lib(), entry)(handle(), C.byref(camera), P(d_kps, with_kps), P(d_cnt, with_kps and use_counts), cap if with_kps else 0, B,
                                      P(d_depth, with_depth), R.KL_ROWS, R.KL_COLS, KL_STEP, KL_FRAME_STRIDE,
                                      P(out["undist"], with_kps), P(out["bearings"], with_kps), P(out["x_right"], with_kps), P(out["depths"], with_kps),
                                      P(d_kl, with_kl), P(d_klcnt, with_kl and use_counts), kl_cap if with_kl else 0,
                                      P(out["kl_depths"], with_kl), P(out["kl_x_right"], with_kl), None)
    sync()
    return status, {k: down(t) for k, t in out.items()}


def kl_expected_bytes(cap, kl_cap, use_counts):
    kd, kx = R.keyline_expected(cap, kl_cap, use_counts)
    want_d, want_x = kl_prefilled(kl_cap)
    want_d, want_x = want_d.copy(), want_x.copy()
    put(want_d, np.float32, 0, kd); put(want_x, np.float32, 0, kx)
    return want_d, want_x


def kp_expected_bytes(cap, kl_cap, use_counts):
    """perspective camera: the four key-point outputs of the oracle, frame by frame, in sentinel-filled buffers"""
    S = R.keyline_scene(cap, kl_cap)
    want = {name: filled(R.KL_B * cap * es + 2 * es) for name, es in KP_OUTPUTS}
    for b in range(R.KL_B):
        n = min(int(S["counts"][b]), cap) if use_counts else cap
        if n == 0:
            continue
        w = O.post_extract(R.PERSPECTIVE10, S["kps"][b, :n], S["depth"][b])
        put(want["undist"], np.uint8, b * cap * 28, w["undist_keypts"].view(np.uint8))
        put(want["bearings"], np.float64, b * cap * 3, w["bearings"])
        put(want["x_right"], np.float32, b * cap, w["stereo_x_right"])
        put(want["depths"], np.float32, b * cap, w["depths"])
    return want


@pytest.mark.parametrize("cap,kl_cap", R.KL_SHAPES)
@pytest.mark.parametrize("entry", list(POST_ENTRIES))
def test_keyline_depth_through_the_batched_device_entries(entry, cap, kl_cap):
    fn, make_camera = POST_ENTRIES[entry]
    camera = make_camera()
    S = R.keyline_scene(cap, kl_cap)
    for use_counts in ((True, False) if (cap, kl_cap) == (257, 257) else (True,)):       # once more with both count pointers NULL
        want_d, want_x = kl_expected_bytes(cap, kl_cap, use_counts)
        pre_d, pre_x = kl_prefilled(kl_cap)
        st, kl_only = run_post_extract(fn, camera, cap, kl_cap, use_counts, False, True)
        assert st == plp.PLP_OK
        same(kl_only["kl_depths"], want_d, "key lines only: kl_depths"); same(kl_only["kl_x_right"], want_x, "key lines only: kl_x_right")
        for name, _ in KP_OUTPUTS:
            assert (kl_only[name] == SENT).all(), name
        st, kp_only = run_post_extract(fn, camera, cap, kl_cap, use_counts, True, False)
        assert st == plp.PLP_OK
        same(kp_only["kl_depths"], pre_d, "key points only: kl_depths"); same(kp_only["kl_x_right"], pre_x, "key points only: kl_x_right")
        st, both = run_post_extract(fn, camera, cap, kl_cap, use_counts, True, True)
        assert st == plp.PLP_OK
        same(both["kl_depths"], want_d, "both: kl_depths"); same(both["kl_x_right"], want_x, "both: kl_x_right")
        for name, es in KP_OUTPUTS:
            same(both[name], kp_only[name], f"both vs key points only: {name}")
            owned = np.zeros(len(kp_only[name]), bool)
            for b in range(R.KL_B):
                n = min(int(S["counts"][b]), cap) if use_counts else cap
                owned[b * cap * es:(b * cap + n) * es] = True
            assert (kp_only[name][~owned] == SENT).all(), name                         # slots above a count, and the tail
        if entry != "model_fisheye":
            for name, want in kp_expected_bytes(cap, kl_cap, use_counts).items():
                same(kp_only[name], want, f"key points only vs the oracle: {name}")


@pytest.mark.parametrize("cap,kl_cap", R.KL_SHAPES)
def test_keyline_depth_host_entry_frame_by_frame(cap, kl_cap):
    S = R.keyline_scene(cap, kl_cap)
    kd, kx = R.keyline_expected(cap, kl_cap, True)
    mt = matcher()
    for camera in (perspective_camera(), model_camera(plp.CAMERA_PERSPECTIVE), model_camera(plp.CAMERA_FISHEYE)):
        for b in range(R.KL_B):
            n, n_kp = min(int(S["kl_counts"][b]), kl_cap), min(int(S["counts"][b]), cap)
            padded = np.full((R.KL_ROWS, R.KL_COLS + 4), -1.0, np.float32)            # a row step of 272 bytes
            padded[:, :R.KL_COLS] = S["depth"][b]
            got = mt.post_extract(camera, S["kps"][b, :n_kp], padded[:, :R.KL_COLS], S["kl"][b, :n], np.full((n, 2), R.KL_PREFILL_DEPTH, np.float32),
                                  np.full((n, 2), R.KL_PREFILL_X_RIGHT, np.float32))
            same(got["kl_depths"], kd[b, :n], f"host kl_depths, frame {b}"); same(got["kl_x_right"], kx[b, :n], f"host kl_x_right, frame {b}")


def test_equirectangular_with_key_lines_or_depth_is_refused_and_writes_nothing():
    cap, kl_cap = 257, 257
    camera = model_camera(plp.CAMERA_EQUIRECTANGULAR)
    pre_d, pre_x = kl_prefilled(kl_cap)
    for with_kps, with_kl, with_depth in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
        st, out = run_post_extract("plp_post_extract_model_device", camera, cap, kl_cap, True, with_kps, with_kl, with_depth)
        assert st == plp.PLP_ERR_UNSUPPORTED, (with_kps, with_kl, with_depth)
        for name, _ in KP_OUTPUTS:
            assert (out[name] == SENT).all(), name
        same(out["kl_depths"], pre_d, "kl_depths"); same(out["kl_x_right"], pre_x, "kl_x_right")


# ------------------------------------------------------------------------------------------------ c. grey conversion
@pytest.mark.parametrize("channels,bgr", [(3, 0), (3, 1), (4, 0), (4, 1)])
def test_grey_conversion_padded_steps_frame_gaps_and_misaligned_bases(channels, bgr):
    rng = np.random.default_rng(31)
    B, rows = R.GRAY_B, R.GRAY_ROWS
    for cols in R.GRAY_COLS:
        src = R.gray_scene(cols, channels)
        want = R.to_gray(src, bgr)
        src_step = cols * channels + 5
        src_fs = rows * src_step + 11
        d_src = up(lay(src.reshape(B, rows, cols * channels), src_step, src_fs, tail=8, rng=rng))
        for gray_step in (cols + 1, cols + 4):
            gray_fs = rows * gray_step + 7
            for off in ((0, 1, 2, 3) if cols in (8, 1024) else (0,)):       # a misaligned base on a 4-divisible width: the byte-store path
                want_buf = lay(want, gray_step, gray_fs, offset=off)
                d_gray = up(filled(len(want_buf)))
                sync()
                plp._check(plp.lib().plp_convert_to_grayscale_device(handle(), d_src.data_ptr(), rows, cols, src_step, src_fs, channels, bgr, B,
                                                                     d_gray.data_ptr() + off, gray_step, gray_fs, None))
                sync()
                same(down(d_gray), want_buf, f"cols {cols}, gray_step {gray_step}, base offset {off}")


# ------------------------------------------------------------------------------------------------ d. true depth
@pytest.mark.parametrize("is_u16", [1, 0])
def test_true_depth_at_the_block_edge_with_special_values(is_u16):
    assert np.float32(1e-40) * np.float32(1000) != 0              # denormals are not flushed in this process: the reference below means what it says
    rng = np.random.default_rng(41)
    B, rows = R.DEPTH_B, R.DEPTH_ROWS
    es = 2 if is_u16 else 4
    for cols in R.DEPTH_COLS:
        v = R.depth_scene(cols, is_u16)
        src_step = cols * es + (6 if is_u16 else 8)
        src_fs = rows * src_step + (10 if is_u16 else 12)
        dst_step = cols * 4 + 12
        dst_fs = rows * dst_step + 20
        d_src = up(lay(v, src_step, src_fs, tail=8, rng=rng))
        for factor in R.DEPTH_FACTORS:
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                want_buf = lay(R.to_true_depth(v, factor), dst_step, dst_fs)
            d_dst = up(filled(len(want_buf)))
            sync()
            plp._check(plp.lib().plp_convert_to_true_depth_device(handle(), d_src.data_ptr(), is_u16, rows, cols, src_step, src_fs, C.c_double(factor), B,
                                                                  d_dst.data_ptr(), dst_step, dst_fs, None))
            sync()
            same(down(d_dst), want_buf, f"cols {cols}, factor {factor}")      # bit patterns: -0.0 -> +0.0, inf, NaN, denormals


# ------------------------------------------------------------------------------------------------ e. colour vote
@pytest.mark.parametrize("rows,cols", R.COLOR_MASKS)
def test_colour_vote_small_masks_block_edge_caps_and_null_optionals(rows, cols):
    rng = np.random.default_rng(51)
    B = R.COLOR_B
    step = cols * 3 + 7
    fs = rows * step + 13
    for cap in R.COLOR_CAPS:
        S = R.color_scene(rows, cols, cap)
        d_mask = up(lay(S["mask"].reshape(B, rows, cols * 3), step, fs, tail=8, rng=rng))
        d_und, d_valid = up(S["undist"]), up(S["valid"])
        for ci, counts in enumerate(R.color_counts(cap)):
            d_cnt = up(counts) if counts is not None else None
            for use_valid in (False, True):
                for check in (1, 0):
                    want = np.full(B * cap + 8, -5, np.int32)
                    want[:B * cap] = R.color_expected(rows, cols, cap, use_valid, ci, check).reshape(-1)      # the kernel owns all cap slots of a frame
                    d_lab = up(np.full(B * cap + 8, -5, np.int32))
                    sync()
                    plp._check(plp.lib().plp_color_vote_device(handle(), d_mask.data_ptr(), rows, cols, step, fs, d_und.data_ptr(),
                                                               d_valid.data_ptr() if use_valid else None, d_cnt.data_ptr() if d_cnt is not None else None, cap, B, check,
                                                               d_lab.data_ptr(), None))
                    sync()
                    same(down(d_lab), want, f"cap {cap}, counts {None if counts is None else counts.tolist()}, valid {use_valid}, check {check}")


# ------------------------------------------------------------------------------------------------ f. remap
@pytest.mark.parametrize("dcols", R.REMAP_DCOLS)
def test_remap_second_block_in_x_padded_map_and_misaligned_destination(dcols):
    rng = np.random.default_rng(61)
    S = R.remap_scene(dcols)
    B, drows = R.REMAP_B, R.REMAP_DROWS
    rows, cols = R.REMAP_SRC
    src_step, map_step, dst_step = cols + 3, dcols * 4 + 16, dcols + 5
    src_fs, dst_fs = rows * src_step + 6, drows * dst_step + 9
    d_src = up(lay(S["src"], src_step, src_fs, tail=8, rng=rng))
    d_mx, d_my = up(lay(S["map_x"][None], map_step, drows * map_step, tail=0, rng=rng)), up(lay(S["map_y"][None], map_step, drows * map_step, tail=0, rng=rng))
    want = np.stack([O.remap_linear(S["src"][b], S["map_x"], S["map_y"]) for b in range(B)])
    want_buf = lay(want, dst_step, dst_fs, offset=1)                     # destination base offset by one byte
    d_dst = up(filled(len(want_buf)))
    sync()
    plp._check(plp.lib().plp_remap_linear_device(handle(), d_src.data_ptr(), rows, cols, src_step, src_fs, d_mx.data_ptr(), d_my.data_ptr(), map_step, drows,
                                                 dcols, B, d_dst.data_ptr() + 1, dst_step, dst_fs, None))
    sync()
    same(down(d_dst), want_buf, f"dst_cols {dcols}")


# ------------------------------------------------------------------------------------------------ g. BoW transform
BOW_OUT = (("word_id", np.uint32), ("node_id", np.uint32), ("bow_word", np.uint32), ("bow_value", np.float64), ("n_bow", np.int32), ("fv_node", np.uint32),
           ("fv_feat", np.uint32), ("n_fv", np.int32))


def bow_buffers(cap):
    B = R.BOW_B
    return {name: filled(((B if name.startswith("n_") else B * cap) + 8) * np.dtype(dt).itemsize) for name, dt in BOW_OUT}


def bow_expected_buffers(name, cap, use_counts):
    want = bow_buffers(cap)
    for b, (wid, nid, bw, bv, fn, ff) in enumerate(R.bow_expected(name, cap, use_counts)):
        put(want["word_id"], np.uint32, b * cap, wid); put(want["node_id"], np.uint32, b * cap, nid)
        put(want["bow_word"], np.uint32, b * cap, bw); put(want["bow_value"], np.float64, b * cap, bv)
        put(want["fv_node"], np.uint32, b * cap, fn); put(want["fv_feat"], np.uint32, b * cap, ff)
        put(want["n_bow"], np.int32, b, [len(bw)]); put(want["n_fv"], np.int32, b, [len(fn)])
    return want


@pytest.mark.parametrize("name", list(R.BOW_VOCABS))
def test_bow_transform_device_entry_at_sort_size_and_group_edges(name):
    assert (plp.TF_IDF, plp.TF, plp.BINARY, plp.L1_NORM, plp.L2_NORM) == (R.TF_IDF, R.TF, R.BINARY, R.L1_NORM, R.L2_NORM)
    V = R.bow_vocab(name)
    v = plp.bow_vocabulary(V["L"], V["parents"], V["is_leaf"], V["descs"], V["weights"], V["weighting"], V["scoring"])
    assert np.array_equal(v.child_offset, V["child_offset"]) and np.array_equal(v.children, V["children"]) and np.array_equal(v.node_word, V["node_word"])
    assert (v.accumulate, v.norm) == (V["accumulate"], V["norm"])
    B = R.BOW_B
    for cap in R.BOW_CAPS:
        d_desc = up(R.bow_scene(name, cap))
        d_cnt = up(R.bow_counts(cap))
        # ragged counts; d_counts NULL; ragged counts with the library's scratch for the per-feature words and nodes
        for use_counts, own_scratch in ((True, True), (False, True), (True, False)):
            want = bow_expected_buffers(name, cap, use_counts)
            out = {k: up(b) for k, b in bow_buffers(cap).items()}
            sync()
            plp._check(plp.lib().plp_bow_transform_device(v._h, d_desc.data_ptr(), d_cnt.data_ptr() if use_counts else None, cap, B, R.BOW_LEVELSUP,
                                                          out["word_id"].data_ptr() if own_scratch else None, out["node_id"].data_ptr() if own_scratch else None,
                                                          out["bow_word"].data_ptr(), out["bow_value"].data_ptr(), out["n_bow"].data_ptr(),
                                                          out["fv_node"].data_ptr(), out["fv_feat"].data_ptr(), out["n_fv"].data_ptr(), None))
            sync()
            for key, _ in BOW_OUT:
                got = down(out[key])
                if not own_scratch and key in ("word_id", "node_id"):
                    assert (got == SENT).all(), key
                else:
                    same(got, want[key], f"cap {cap}, counts {use_counts}, scratch {own_scratch}: {key}")
            if use_counts:      # what the census of the CPU test says about frames 0 and 3, in the device's own counts
                assert down(out["n_bow"], np.int32)[[0, 3]].tolist() == [1, 0] and down(out["n_fv"], np.int32)[[0, 3]].tolist() == [cap, 0]
