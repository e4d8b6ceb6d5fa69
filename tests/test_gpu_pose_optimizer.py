"""optimize::pose_optimizer / pose_optimizer_extended_line on the device (plp_pose_optimize_device / _host, csrc/pose_opt_kernels.hip) against
the CPU build of the same header (plp.model_pose_optimize, which tests/test_pose_optimizer_cpu.py holds bit for bit to the restatement
tests/pose_optimizer_ref.py): every output bit for bit on sentinel-filled arrays, at the smallest shapes at which the
kernels can go wrong -- numbers of observations around the minimum of five, the wave (64) and the pass tile (256) up to its third tile, dense
and with holes that move ranks across those edges, numbers of lines around the wave and the tile, 8192 slots, ragged frames that reach both
statuses, the early breaks, rejected steps and non-finite systems in one call for both camera models and the three set-ups, trial and iteration
counts, absent optional outputs and inputs, and two calls back to back on one stream."""
import numpy as np
import pytest

import pose_optimizer_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25}
OPTIONAL = ("trial_info", "trial_chi2")
TILE = 256   # kPoseTile of csrc/pose_opt_kernels.hip: edges per pass tile, one per lane


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(B, N, L, T):
    return {k: np.full((B,) + shape(N, L, T), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.POSE_OPT_OUTPUTS.items()}


def same_values(a, b):
    """the same bits, a NaN equal to any NaN (no output's meaning carries a NaN's sign or payload)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.nan_to_num(a, nan=0.0).tobytes() == np.nan_to_num(b, nan=0.0).tobytes()


def shapes(P):
    B, N = P["valid"].shape
    return B, N, 0 if P["lines"] is None else P["lines"]["valid"].shape[1]


def enqueue_device(mt, P, T=4, I=10, skip_optional=False, x_right=True, counts=True, stream=None):
    """plp_pose_optimize_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    B, N, L = shapes(P)

    def d(v):
        v = np.ascontiguousarray(v)
        return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(B, N, L, T).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL) and v.numel()}
    ln = P["lines"]
    dev = dict(pose=d(P["pose_in"]), valid=d(P["valid"]), undist=d(P["undist"]), pos_w=d(P["pos_w"]), x_right=d(P["x_right"]), counts=d(P["counts"]))
    kw = {}
    if ln is not None:
        dev.update(lv=d(ln["valid"]), kl=d(ln["keylines"]), lw=d(ln["pos_w"]), lc=d(ln["counts"]))
        kw = dict(l_cap=L, line_valid=dev["lv"], keylines=dev["kl"], pos_w_lines=dev["lw"], inv_level_sigma_sq_lsd=ln["inv_level_sigma_sq_lsd"],
                  line_counts=dev["lc"] if counts else None)
    mt.pose_optimize_device(P["camera"], P["setup_type"], B, N, dev["pose"], dev["valid"], dev["undist"], dev["pos_w"], S.INV_SIGMA_SQ, passed,
                            x_right=dev["x_right"] if x_right else None, counts=dev["counts"] if counts else None, num_trials=T, num_each_iter=I,
                            pose_stride=P["pose_in"].shape[1], stream=stream, **kw)
    return o, dev


def model_args(P, T, I, x_right=True, counts=True):
    a = S.call_args(P, num_trials=T, num_each_iter=I)
    if not x_right:
        a["x_right"] = None
    if not counts:
        a["counts"] = None
        if a["lines"] is not None:
            a["lines"] = dict(a["lines"], counts=None)
    return a


def compare(want, got, skip_optional=False):
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == SENT[got[k].dtype]).all(), ("an output that was not passed was written", k)
        else:
            assert same_values(want[k], got[k]), (k, want[k], got[k])


def check(mt, P, T=4, I=10, host=True, **opt):
    import torch
    B, N, L = shapes(P)
    a = model_args(P, T, I, opt.get("x_right", True), opt.get("counts", True))
    want = plp.model_pose_optimize(out=sentinels(B, N, L, T), **a)
    if opt.get("counts", True):
        for b in range(B):                                        # the model itself leaves the slots above a count alone
            assert (want["outlier"][b, int(P["counts"][b]):] == SENT[np.dtype(np.uint8)]).all()
    o, _ = enqueue_device(mt, P, T, I, **opt)
    torch.cuda.synchronize()
    compare(want, {k: v.cpu().numpy() for k, v in o.items()}, opt.get("skip_optional", False))
    if host:
        compare(want, mt.pose_optimize(out=sentinels(B, N, L, T), **a))
    return want


EDGE_COUNTS = [4, 5, 6, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


@pytest.mark.parametrize("holes", [0.0, 0.3])
@pytest.mark.parametrize("setup", [S.MONO, S.RGBD])
def test_observation_counts_around_the_minimum_the_wave_and_the_tiles(mt, setup, holes):
    frames = [S.make_frame(100 + n, n, setup=setup, noise=1.0, outlier_share=0.15, rot=0.05, trans=0.1) for n in EDGE_COUNTS]
    r = check(mt, S.pack(frames, holes=holes, seed=5))
    assert r["num_init_obs"].tolist() == EDGE_COUNTS and r["status"].tolist() == [plp.POSE_OPT_TOO_FEW_OBS] + [plp.POSE_OPT_OK] * (len(EDGE_COUNTS) - 1)


@pytest.mark.parametrize("holes", [0.0, 0.3])
def test_line_counts_around_the_wave_and_the_tile(mt, holes):
    frames = [S.make_frame(200 + k, 40, setup=S.STEREO, n_lines=k, noise=0.7, outlier_share=0.15, rot=0.05, trans=0.1) for k in (0, 1, 63, 64, 65, TILE + 1)]
    check(mt, S.pack(frames, holes=holes, seed=6))


def test_8192_slots_with_a_few_hundred_in_use(mt):
    frames = [S.make_frame(300 + i, 300, setup=S.RGBD, n_lines=120, noise=1.0, outlier_share=0.1, rot=0.05, trans=0.1) for i in range(2)]
    P = S.pack(frames, n_cap=8192, l_cap=8192, holes=0.9, seed=7)
    assert P["counts"].max() > 2900 and P["lines"]["counts"].max() > 1100
    check(mt, P)


@pytest.mark.parametrize("model", ["perspective", "fisheye"])
@pytest.mark.parametrize("setup", [S.MONO, S.STEREO, S.RGBD])
def test_ragged_frames_of_the_census_in_one_call(mt, setup, model):
    r = check(mt, S.pack(S.census_frames(model, setup), holes=0.25, seed=8))
    assert set(r["status"].tolist()) == {plp.POSE_OPT_OK, plp.POSE_OPT_TOO_FEW_OBS}
    ends = r["trial_info"][:, :, 3]
    assert (ends == 0).any() and (ends == plp.POSE_OPT_END_TRIES).any() and (r["trial_info"][:, :, 1] > 0).any()


@pytest.mark.parametrize("T,I", [(1, 1), (1, 10), (2, 1), (2, 10), (4, 1)])
def test_trial_and_iteration_counts(mt, T, I):
    frames = [S.make_frame(400 + i, 30 + 40 * i, setup=S.STEREO, n_lines=7 * i, noise=1.0, outlier_share=0.2, rot=0.08, trans=0.2) for i in range(3)]
    check(mt, S.pack(frames, holes=0.2, seed=9), T=T, I=I, host=False)


def test_absent_optional_outputs_and_inputs(mt):
    frames = [S.make_frame(500 + i, 20 + 50 * i, setup=S.MONO, n_lines=5, noise=1.0, outlier_share=0.2) for i in range(3)]
    P = S.pack(frames, seed=10)
    check(mt, P, skip_optional=True, host=False)
    check(mt, P, x_right=False, host=False)
    full = S.pack(frames, seed=10)
    full["valid"][:] = np.where(np.arange(full["valid"].shape[1])[None] < full["counts"][:, None], full["valid"], 0)   # NULL counts: every slot is looked at
    full["lines"]["valid"][:] = np.where(np.arange(full["lines"]["valid"].shape[1])[None] < full["lines"]["counts"][:, None], full["lines"]["valid"], 0)
    check(mt, full, counts=False)


def test_two_calls_back_to_back_on_one_stream(mt):
    import torch
    P1 = S.pack([S.make_frame(600 + i, 80, setup=S.RGBD, n_lines=10, noise=1.0, outlier_share=0.2) for i in range(3)], holes=0.2, seed=11)
    P2 = S.pack([S.make_frame(610 + i, 300, setup=S.RGBD, n_lines=4, noise=0.5, outlier_share=0.1) for i in range(2)], holes=0.1, seed=12)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        o1, keep1 = enqueue_device(mt, P1, stream=st)
        o2, keep2 = enqueue_device(mt, P2, stream=st)
    st.synchronize()
    for P, o in ((P1, o1), (P2, o2)):
        B, N, L = shapes(P)
        compare(plp.model_pose_optimize(out=sentinels(B, N, L, 4), **model_args(P, 4, 10)), {k: v.cpu().numpy() for k, v in o.items()})


def test_the_equirectangular_camera_is_unsupported_and_nothing_is_written(mt):
    import torch
    P = S.pack([S.make_frame(700, 30)])
    P["camera"].model = plp.CAMERA_EQUIRECTANGULAR
    with pytest.raises(plp.PlpError) as e:
        enqueue_device(mt, P)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    B, N, L = shapes(P)
    out = sentinels(B, N, L, 4)
    with pytest.raises(plp.PlpError) as e:
        mt.pose_optimize(out=out, **model_args(P, 4, 10))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == SENT[v.dtype]).all(), k


def test_no_frames(mt):
    P = S.pack([S.make_frame(800, 10)])
    a = model_args(P, 4, 10)
    for k in ("pose_in", "valid", "undist", "pos_w", "x_right", "counts"):
        a[k] = a[k][:0]
    r = mt.pose_optimize(**a)
    assert r["status"].shape == (0,) and r["pose"].shape == (0, 15)
    mt.pose_optimize_device(P["camera"], S.MONO, 0, 10, None, None, None, None, S.INV_SIGMA_SQ, {})
