"""optimize::global_bundle_adjuster and the loop adjuster's map update on the device (plp_global_ba_device / _host, plp_loop_ba_propagate_*,
csrc/global_ba_kernels.hip) against the CPU build of the same header (plp.model_global_ba / model_loop_ba_propagate / model_chol_dense, which
tests/test_global_ba_cpu.py holds bit for bit to the restatement tests/global_ba_ref.py): every output bit for bit on
sentinel-filled arrays, at the smallest shapes at which the kernels can go wrong.  The widths the kernels use: PANEL columns of a Cholesky panel and
of a block of the substitutions, ROWS rows per workgroup of the rows-below launch, the workgroup of 256 lanes (WG: one item per lane of every grid,
the LDS tile of the chains) and the wave of 64 (the ballot scan that builds a pose's edge list)."""
import numpy as np
import pytest

import global_ba_ref as REF
import global_ba_scene as GS
import local_ba_scene as LS
from plp import plp

pytestmark = pytest.mark.gpu
PANEL, ROWS, WG, WAVE = 32, 64, 256, 64       # PLP_GLOBAL_BA_PANEL, PLP_GLOBAL_BA_ROWS of include/plp_front.h, kGbThreads of csrc/global_ba.hpp, the wave
OPTIONAL = ("info", "chi2")
TABLES = ("pose", "kf_erased", "kf_is_origin", "undist", "x_right", "counts", "pos_w", "lm_erased", "obs_offsets", "obs_kf", "obs_idx")


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def test_the_header_exports_the_widths():
    assert (plp.GLOBAL_BA_PANEL, plp.GLOBAL_BA_ROWS) == (PANEL, ROWS)
    h = (plp.ROOT / "include" / "plp_front.h").read_text()
    assert f"#define PLP_GLOBAL_BA_PANEL {PANEL} " in h and f"#define PLP_GLOBAL_BA_ROWS {ROWS} " in h


def host_model(sc, **kw):
    return plp.model_global_ba(**GS.call_args(sc, **kw), out=GS.sentinel_out(sc))


def dev(v):
    import torch
    if v is None:
        return None
    v = np.ascontiguousarray(v)
    return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()


def run_device(mt, sc, skip_optional=False, keep=None, stop=None, **kw):
    """plp_global_ba_device on sentinel-filled device outputs; returns the outputs as numpy arrays"""
    import torch
    F, L, T = GS.dims(sc)
    a = GS.call_args(sc, **kw)
    o = {k: dev(v) for k, v in GS.sentinel_out(sc).items()}
    if keep is not None:
        keep.update(o)
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL) and v.numel()}
    d = {k: dev(a[k]) for k in TABLES}
    mt.global_ba_device(a["camera"], a["setup_type"], F, L, T, sc["undist"].shape[1], d["pose"], d["undist"], d["pos_w"], d["obs_offsets"], d["obs_kf"], d["obs_idx"],
                        a["inv_level_sigma_sq"], passed, x_right=d["x_right"], counts=d["counts"], kf_erased=d["kf_erased"], kf_is_origin=d["kf_is_origin"],
                        lm_erased=d["lm_erased"], pose_stride=sc["pose"].shape[1], num_iter=a.get("num_iter", 10), use_huber_kernel=a.get("use_huber_kernel", True), stop=stop)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check(mt, sc, skip_optional=False, **kw):
    want = host_model(sc, **kw)
    got = run_device(mt, sc, skip_optional=skip_optional, **kw)
    sent = GS.sentinel_out(sc)
    for k in want:
        assert LS.same({k: got[k]}, {k: sent[k] if (skip_optional and k in OPTIONAL) else want[k]}), k
    return want


# 6 P rows: P = 5 / 6 around one panel (30 / 36), 10 / 11 around two (60 / 66), 16 / 17 around the first workgroup of rows below the first panel (96 / 102
# = PANEL + ROWS + 6), 65 the first problem D17 refuses
@pytest.mark.parametrize("P", [0, 1, 5, 6, 10, 11, 16, 17, 65])
def test_free_key_frames_at_the_panel_and_row_group_boundaries(mt, P):
    sc = GS.make(500 + P, P, 60 + 4 * P, noise=0.6, per_kf=20)
    want = check(mt, sc, num_iter=3, use_huber_kernel=P % 2 == 0)
    assert want["status"][0] == plp.GLOBAL_BA_OK and want["kf_optimized"].sum() == P + 1 and want["info"][0] == 3


def test_several_panels_times_several_row_groups(mt):
    """P = 130 with about 20 observations per key frame: 780 rows, 25 panels, up to 12 row groups"""
    sc = GS.make(640, 130, 650, noise=0.5, per_kf=20)
    F, L, T = GS.dims(sc)
    want = check(mt, sc, num_iter=2, use_huber_kernel=False)
    assert want["status"][0] == plp.GLOBAL_BA_OK and want["info"][2] >= 2 and 15 < T / F < 25


@pytest.mark.parametrize("n", [1, PANEL - 1, PANEL, PANEL + 1, 2 * PANEL - 1, 2 * PANEL + 1, PANEL + ROWS, PANEL + ROWS + 1, 402, 780])
def test_panel_cholesky_equals_the_host_form(mt, n):
    """the panel kernels alone (plp_chol_dense_host) against the column-by-column host form, bit for bit, at every size at which a panel, a block of the
    substitutions or a row group begins; and a pivot that fails in the last panel"""
    rng = np.random.default_rng(n)
    B = rng.normal(size=(n, n)) / np.sqrt(n)
    A, b = B @ B.T, rng.normal(size=n)
    x, ok = mt.chol_dense(A, b, 0.05)
    wx, wok = plp.model_chol_dense(A, b, 0.05)
    assert ok and wok and x.tobytes() == wx.tobytes()
    A[n - 1, n - 1] = -1.0
    x, ok = mt.chol_dense(A, b, 0.05)
    assert not ok and not plp.model_chol_dense(A, b, 0.05)[1] and not x.any()


@pytest.mark.parametrize("T", [WAVE - 1, WAVE + 1, WG - 1, WG + 1])
def test_observation_counts_around_the_wave_and_the_workgroup(mt, T):
    from test_gpu_local_ba import cut
    sc = cut(GS.make(700 + T, 3, 200, noise=0.8, outliers=8, obs_share=0.7), T)
    want = check(mt, sc, num_iter=4)
    assert want["status"][0] == plp.GLOBAL_BA_OK


@pytest.mark.parametrize("L", [WG - 1, WG, WG + 1])
def test_landmark_counts_around_the_workgroup(mt, L):
    sc = GS.make(800 + L, 2, L, setup=GS.MONO, noise=0.8, outliers=10, obs_share=0.4)
    want = check(mt, sc, num_iter=4)
    assert want["lm_optimized"].sum() >= 150 and want["lm_optimized"][WG - 2:].any()


def test_key_frame_table_larger_than_a_workgroup(mt):
    """F = 300: the scene's key frames spread over the table, the other rows observe nothing and get the converted input"""
    sc = GS.make(901, 6, 60, noise=0.6)
    rows = np.array([0, 3, 255, 256, 257, 290, 299])
    sp = LS.spread(sc, rows, 300)
    want = check(mt, sp, num_iter=4)
    assert want["kf_optimized"].all() and want["status"][0] == plp.GLOBAL_BA_OK


@pytest.mark.parametrize("name", ["mono_huber", "fisheye_stereo", "rejected", "at_truth", "no_information", "behind", "nan", "holes", "origin_only", "no_edges"])
def test_census_scenes(mt, name):
    """Huber on and off, RGB-D fisheye and monocular perspective, the scenes that fail solves, end by rho == 0 and by the ten tries, NO_EDGES"""
    sc, it, hub = GS.census()[name]
    check(mt, sc, num_iter=it, use_huber_kernel=hub)


def test_rgbd_fisheye_and_odd_strides_and_absent_optionals(mt):
    sc = GS.make(950, 7, 90, model="fisheye", noise=0.7, outliers=6, kp_stride=131, pose_stride=17)
    sc["counts"] = None
    sc["kf_erased"] = None
    sc["lm_erased"] = None
    check(mt, sc, skip_optional=True, num_iter=4)


def test_two_calls_back_to_back_the_second_smaller(mt):
    big = GS.make(960, 12, 150, noise=0.6)
    small = GS.make(961, 2, 20, noise=0.6)
    check(mt, big, num_iter=3)
    check(mt, small, num_iter=3)
    check(mt, GS.census()["no_edges"][0], num_iter=3)


def test_host_pointer_entry_equals_the_device_entry(mt):
    sc = GS.make(970, 9, 100, setup=GS.STEREO, noise=0.6, outliers=5)
    want = check(mt, sc, num_iter=4)
    got = mt.global_ba(**GS.call_args(sc, num_iter=4), out=GS.sentinel_out(sc))
    assert LS.same(got, want)
    some = mt.global_ba(**GS.call_args(sc, num_iter=4), outputs=(), out=GS.sentinel_out(sc, ("status", "kf_optimized", "lm_optimized", "pose", "pos_w")))
    assert set(some) == {"status", "kf_optimized", "lm_optimized", "pose", "pos_w"} and LS.same(some, {k: want[k] for k in some})


def test_refusals_write_nothing(mt):
    import torch
    sc = GS.make(980, 3, 30, noise=0.6)
    cam = LS.PS.camera("perspective")
    cam.model = plp.CAMERA_EQUIRECTANGULAR
    for kw, status in ((dict(num_iter=0), plp.PLP_ERR_INVALID_ARG), (dict(camera=cam), plp.PLP_ERR_UNSUPPORTED), (dict(setup_type=-1), plp.PLP_ERR_INVALID_ARG)):
        keep = {}
        with pytest.raises(plp.PlpError) as e:
            run_device(mt, sc, keep=keep, **kw)
        torch.cuda.synchronize()
        assert e.value.status == status and LS.same({k: v.cpu().numpy() for k, v in keep.items()}, GS.sentinel_out(sc)), kw
        out = GS.sentinel_out(sc)
        with pytest.raises(plp.PlpError):
            mt.global_ba(**GS.call_args(sc, **kw), out=out)
        assert LS.same(out, GS.sentinel_out(sc))


def test_stop_set_before_the_call(mt):
    sc = GS.make(990, 3, 30, noise=0.6)
    stop = np.ones(1, np.int32)
    want = GS.sentinel_out(sc)
    want["status"][0] = plp.GLOBAL_BA_STOPPED
    assert LS.same(run_device(mt, sc, stop=stop, num_iter=4), want)
    assert LS.same(mt.global_ba(**GS.call_args(sc, num_iter=4, stop=stop), out=GS.sentinel_out(sc)), want)
    stop[0] = 0
    assert LS.same(run_device(mt, sc, stop=stop, num_iter=4), host_model(sc, num_iter=4))


# ---- the map update
def prop_device(mt, Tr):
    import torch
    F, L = len(Tr["pose"]), len(Tr["pos_w"])
    o = {k: dev(v) for k, v in GS.prop_sentinel(Tr).items()}
    d = {k: dev(v) for k, v in Tr.items()}
    mt.loop_ba_propagate_device(F, L, d["pose"], d["kf_parent"], d["kf_optimized"], d["pose_after"], d["pos_w"], d["ref_kf"], d["lm_optimized"], d["pos_after"], o,
                                kf_erased=d["kf_erased"], kf_is_origin=d["kf_is_origin"], lm_erased=d["lm_erased"], pose_stride=Tr["pose"].shape[1])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.timeout(20)
@pytest.mark.parametrize("name", GS.TREES)
def test_propagation_equals_the_restatement(mt, name):
    """every tree scene, the cycle and the broken link included (every walk is bounded by F: both return), _device and _host"""
    Tr = GS.tree(name)
    want, _ = GS.prop_expected(Tr)
    assert LS.same(prop_device(mt, Tr), want)
    assert LS.same(mt.loop_ba_propagate(**Tr, out=GS.prop_sentinel(Tr)), want)


def test_propagation_over_more_than_a_workgroup(mt):
    """F = 300 in a chain whose every third key frame is unoptimised, L = 700"""
    Tr = GS.tree("leaves", seed=9, n_lm=700)
    F = 300
    rng = np.random.default_rng(3)
    big = GS.tree("leaves", seed=10, n_lm=700)
    reps = (F + 6) // 7
    for k in ("pose", "pose_after"):
        big[k] = np.tile(Tr[k], (reps, 1))[:F] + rng.normal(size=(F, 15)) * 1e-3
    big["kf_parent"] = np.arange(-1, F - 1).astype(np.int32)
    big["kf_optimized"] = (np.arange(F) % 3 != 2).astype(np.uint8)
    big["kf_erased"] = np.zeros(F, np.uint8)
    big["kf_is_origin"] = np.zeros(F, np.uint8); big["kf_is_origin"][0] = 1
    big["ref_kf"] = rng.integers(-1, F + 1, 700).astype(np.int32)
    want = plp.model_loop_ba_propagate(**big, out=GS.prop_sentinel(big))
    assert (want["kf_status"] == REF.KF_PROPAGATED).sum() == F // 3 and LS.same(prop_device(mt, big), want)
