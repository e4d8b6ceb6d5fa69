"""optimize::transform_optimizer on the device (plp_transform_optimize_device / _host, csrc/transform_opt_kernels.hip) against the CPU build of the
same header (plp.model_transform_optimize, which tests/test_transform_optimizer_cpu.py holds bit for bit to the restatement
tests/transform_optimizer_ref.py): every output bit for bit on sentinel-filled arrays, at the smallest shapes at which
the kernels can go wrong -- numbers of matches around the minimum of ten, the half wave, the wave and the pass tile (128 matches, 256 edges) up to
its third tile, dense and with holes that move ranks across those edges, 8192 slots, ragged problems that reach both statuses and the non-finite
systems in one call for both camera models and fix_scale on and off, iteration counts, absent optional outputs and counts, and two calls back to
back on one stream."""
import numpy as np
import pytest

import transform_optimizer_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25}
OPTIONAL = ("world_to_1", "round_info", "round_chi2")
TILE = 128   # kTfTile of csrc/transform_opt_kernels.hip: matches per pass tile, two edges each, one edge per lane


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, N):
    return {k: np.full((P,) + shape(N), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.TRANSFORM_OPT_OUTPUTS.items()}


def same_values(a, b):
    """the same bits, a NaN equal to any NaN (no output's meaning carries a NaN's sign or payload)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.nan_to_num(a, nan=0.0).tobytes() == np.nan_to_num(b, nan=0.0).tobytes()


def enqueue_device(mt, A, num_iter=10, skip_optional=False, counts=True, sig1=S.INV_SIGMA_SQ, stream=None):
    """plp_transform_optimize_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    P, N = A["valid"].shape

    def d(v):
        v = np.ascontiguousarray(v)
        return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(P, N).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL) and v.numel()}
    dev = {k: d(A[k]) for k in ("valid", "pos_w_1", "pos_w_2", "undist_1", "undist_2", "pose_1", "pose_2", "rot_12", "trans_12", "scale_12", "counts")}
    mt.transform_optimize_device(A["camera"], A["fix_scale"], P, N, dev["valid"], dev["pos_w_1"], dev["pos_w_2"], dev["undist_1"], dev["undist_2"], dev["pose_1"],
                                 dev["pose_2"], dev["rot_12"], dev["trans_12"], dev["scale_12"], sig1, S.INV_SIGMA_SQ, passed,
                                 counts=dev["counts"] if counts else None, num_iter=num_iter, stream=stream)
    return o, dev


def compare(want, got, skip_optional=False):
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == SENT[got[k].dtype]).all(), ("an output that was not passed was written", k)
        else:
            assert same_values(want[k], got[k]), (k, want[k], got[k])


def check(mt, A, num_iter=10, host=True, skip_optional=False, counts=True, sig1=S.INV_SIGMA_SQ):
    import torch
    P, N = A["valid"].shape
    a = S.call_args(A, num_iter=num_iter, inv_level_sigma_sq_1=sig1)
    if not counts:
        a["counts"] = None
    want = plp.model_transform_optimize(out=sentinels(P, N), **a)
    if counts:
        for p in range(P):                                        # the model itself leaves the slots above a count alone
            assert (want["kept"][p, int(A["counts"][p]):] == SENT[np.dtype(np.uint8)]).all()
    o, _ = enqueue_device(mt, A, num_iter, skip_optional, counts, sig1)
    torch.cuda.synchronize()
    compare(want, {k: v.cpu().numpy() for k, v in o.items()}, skip_optional)
    if host:
        compare(want, mt.transform_optimize(out=sentinels(P, N), **a))
    return want


EDGE_COUNTS = [0, 1, 9, 10, 11, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


@pytest.mark.parametrize("holes", [0.0, 0.3])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_match_counts_around_the_minimum_the_waves_and_the_tiles(mt, fix_scale, holes):
    pr = [S.make_problem(100 + n, n, fix_scale=fix_scale, noise=1.0, outlier_share=0.15, rot=0.05, trans=0.1) for n in EDGE_COUNTS]
    r = check(mt, S.pack(pr, holes=holes, seed=5))
    assert r["num_valid"].tolist() == EDGE_COUNTS
    assert (r["status"][:3] == plp.TRANSFORM_OPT_TOO_FEW_INLIERS).all() and (r["status"][5:] == plp.TRANSFORM_OPT_OK).all()


def test_8192_slots_with_a_handful_valid(mt):
    pr = [S.make_problem(300 + i, 60 + 90 * i, noise=1.0, outlier_share=0.1, rot=0.05, trans=0.1) for i in range(2)]
    A = S.pack(pr, n_cap=8192, holes=0.98, seed=7)
    assert A["counts"].max() > 7000
    check(mt, A)


@pytest.mark.parametrize("model", ["perspective", "fisheye"])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_ragged_problems_of_the_census_in_one_call(mt, fix_scale, model):
    r = check(mt, S.pack(S.census_problems(model, fix_scale), holes=0.25, seed=8))
    assert set(r["status"].tolist()) == {plp.TRANSFORM_OPT_OK, plp.TRANSFORM_OPT_TOO_FEW_INLIERS}
    ends = r["round_info"][:, :, 3]
    assert (ends == 0).any() and (ends == plp.POSE_OPT_END_TRIES).any() and (ends == plp.POSE_OPT_END_RHO_ZERO).any() and (r["round_info"][:, :, 1] > 0).any()
    assert np.isnan(r["round_chi2"]).any()                        # the non-finite systems


def test_a_nan_at_the_end_of_round_2(mt):
    r = check(mt, S.pack([S.nan_in_round_2_problem(), S.make_problem(350, 70, noise=0.5)], holes=0.1, seed=9), sig1=S.INV_SIGMA_SQ_W0)
    assert r["status"][0] == plp.TRANSFORM_OPT_OK and r["round_info"][0, 1, 1] > 0


@pytest.mark.parametrize("num_iter", [1, 10])
def test_iteration_counts(mt, num_iter):
    pr = [S.make_problem(400 + i, 30 + 60 * i, noise=1.0, outlier_share=0.2, rot=0.08, trans=0.2) for i in range(3)]
    check(mt, S.pack(pr, holes=0.2, seed=10), num_iter=num_iter, host=False)


def test_absent_optional_outputs_and_counts(mt):
    pr = [S.make_problem(500 + i, 20 + 50 * i, noise=1.0, outlier_share=0.2) for i in range(3)]
    A = S.pack(pr, seed=11)
    check(mt, A, skip_optional=True, host=False)
    full = S.pack(pr, seed=11)
    full["valid"][:] = np.where(np.arange(full["valid"].shape[1])[None] < full["counts"][:, None], full["valid"], 0)   # NULL counts: every slot is looked at
    check(mt, full, counts=False)


def test_two_calls_back_to_back_on_one_stream(mt):
    import torch
    A1 = S.pack([S.make_problem(600 + i, 80, noise=1.0, outlier_share=0.2) for i in range(3)], holes=0.2, seed=12)
    A2 = S.pack([S.make_problem(610 + i, 300, fix_scale=True, noise=0.5, outlier_share=0.1) for i in range(2)], holes=0.1, seed=13)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        o1, keep1 = enqueue_device(mt, A1, stream=st)
        o2, keep2 = enqueue_device(mt, A2, stream=st)
    st.synchronize()
    for A, o in ((A1, o1), (A2, o2)):
        P, N = A["valid"].shape
        compare(plp.model_transform_optimize(out=sentinels(P, N), **S.call_args(A)), {k: v.cpu().numpy() for k, v in o.items()})


def test_the_equirectangular_camera_is_unsupported_and_nothing_is_written(mt):
    import torch
    A = S.pack([S.make_problem(700, 30)])
    A["camera"].model = plp.CAMERA_EQUIRECTANGULAR
    with pytest.raises(plp.PlpError) as e:
        enqueue_device(mt, A)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    out = sentinels(*A["valid"].shape)
    with pytest.raises(plp.PlpError) as e:
        mt.transform_optimize(out=out, **S.call_args(A))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == SENT[v.dtype]).all(), k


def test_no_problems(mt):
    A = S.pack([S.make_problem(800, 10)])
    a = S.call_args(A)
    for k in ("valid", "pos_w_1", "pos_w_2", "undist_1", "undist_2", "pose_1", "pose_2", "rot_12", "trans_12", "scale_12", "counts"):
        a[k] = a[k][:0]
    r = mt.transform_optimize(**a)
    assert r["status"].shape == (0,) and r["rot_12"].shape == (0, 9)
    mt.transform_optimize_device(A["camera"], False, 0, 10, None, None, None, None, None, None, None, None, None, None, S.INV_SIGMA_SQ, S.INV_SIGMA_SQ, {})
