"""bearing_vector::reconstruct_with_E on the device (plp_two_view_pose_device / _host, csrc/two_view_kernels.hip) against the CPU build of the
same header (plp.model_two_view_pose, which tests/test_two_view_pose_cpu.py holds bit for bit to the restatement; DESIGN.md section 5, D24 items
c, f, g): every output bit for bit on sentinel-filled arrays, for the three cameras, at slot counts around the 256-slot pass of the workgroup
(63, 64, 65, 255, 256, 257, 513) with holes, numbers of valid points around the rank of the order statistic (50, 51, 52), ragged problems
with all five statuses in one call, depth_is_positive on and off, the optional output absent, two calls back to back on one stream, and
initializer_step.run: the RANSAC and the pose chained on one stream without the host."""
import importlib

import numpy as np
import pytest

import two_view_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25, np.dtype(np.float32): np.float32(-321.5)}


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap):
    return {k: np.full((P,) + shape(n_cap), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.TWO_VIEW_OUTPUTS.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def inputs(problems, model, seed=5):
    """the packed tables of problems of one camera and the RANSAC's outputs (host build) that feed the pose entry"""
    qs = [dict(q, iters=8, samples=q["samples"][:8]) for q in problems]
    a = S.pose_pack(qs)
    e = plp.model_essential_ransac(a["bearing_1"], a["bearing_2"], a["match"], iters=16, seed=seed, counts_1=a["counts_1"], counts_2=a["counts_2"])
    inl = np.where(np.arange(a["match"].shape[1])[None] < a["counts_1"][:, None], e["inliers"], 1).astype(np.uint8)   # flags above a count are not read
    cam = plp.camera_model(S.CAMERAS[model])
    pos = (cam, e["E_21"], inl, a["match"], a["bearing_1"], a["bearing_2"], a["undist_1"], a["undist_2"])
    kw = dict(in_status=e["status"], counts_1=a["counts_1"], counts_2=a["counts_2"], img_bounds=S.bounds(S.ref_camera(model)))
    return pos, kw


def enqueue_device(mt, pos, kw, skip_optional=False, **params):
    import torch
    cam, arrays = pos[0], pos[1:]
    P, n_cap = arrays[2].shape
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(P, n_cap).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k == "hyp_is_triangulated")}
    dev = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda() if v.dtype == plp.KP_DTYPE else d(v) for v in arrays]
    dkw = {k: d(kw[k]) for k in ("in_status", "counts_1", "counts_2")}
    mt.two_view_pose_device(cam, P, n_cap, arrays[4].shape[1], *dev, passed, img_bounds=kw["img_bounds"], **dkw, **params)
    return o, (dev, dkw)


def check(mt, problems, model, host=True, skip_optional=False, **params):
    import torch
    pos, kw = inputs(problems, model)
    P, n_cap = pos[3].shape
    want = plp.model_two_view_pose(*pos, out=sentinels(P, n_cap), **kw, **params)
    o, _ = enqueue_device(mt, pos, kw, skip_optional, **params)
    torch.cuda.synchronize()
    for k in want:
        got = o[k].cpu().numpy()
        if skip_optional and k == "hyp_is_triangulated":
            assert (got == SENT[got.dtype]).all(), "an output that was not passed was written"
        else:
            assert same_bits(got, want[k]), ("device", k, got, want[k])
    if host:
        h = mt.two_view_pose(*pos, out=sentinels(P, n_cap), **kw, **params)
        for k in want:
            assert same_bits(h[k], want[k]), ("host entry", k)
    return want


@pytest.mark.parametrize("model", S.MODELS)
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
def test_slot_counts_around_every_edge(mt, model, n):
    dense = S.pose_problem(700 + n, n, model, noise=5e-4, mismatch=0.2)
    holes = S.pose_problem(800 + n, n, model, n_slots=2 * n + 7, noise=5e-4)
    for dip in (False, True):
        w = check(mt, [dense, holes], model, host=not dip, depth_is_positive=dip)
    assert w["num_valid"].max() > 0


@pytest.mark.parametrize("n", [50, 51, 52])
def test_numbers_of_valid_points_around_the_rank_of_the_order_statistic(mt, n):
    """exact matches only: all n are valid under the true hypothesis, and the parallax is the value of rank min(50, n - 1)"""
    q = S.pose_problem(900 + n, n, "equirectangular", n_slots=n + 9, noise=0.0)
    w = check(mt, [q], "equirectangular", min_num_triangulated=40, parallax_deg_thr=0.1)
    assert w["status"][0] == plp.TWO_VIEW_OK and w["num_valid"][0].max() == n


def test_ragged_problems_reach_all_five_statuses_in_one_call(mt):
    sc = S.pose_scenes()
    qs = [S.pose_problem(600 + 2, 200, "equirectangular", n_slots=210, noise=5e-4), sc["mirrored"], sc["all_mismatched"],
          S.pose_problem(455, 30, "equirectangular", n_slots=40, noise=5e-4), S.pose_problem(458, 150, "equirectangular", noise=1e-4, kind="near_rotation"),
          S.pose_problem(459, 5, "equirectangular", n_slots=9)]
    w = check(mt, qs, "equirectangular")
    assert set(w["status"].tolist()) == {plp.TWO_VIEW_OK, plp.TWO_VIEW_NO_SOLUTION, plp.TWO_VIEW_TOO_FEW_TRIANGULATED, plp.TWO_VIEW_AMBIGUOUS,
                                         plp.TWO_VIEW_SMALL_PARALLAX}, w["status"]


def test_the_scenes_of_the_cpu_census(mt):
    sc = S.pose_scenes()
    for model in S.MODELS:
        check(mt, [q for q in sc.values() if q["camera"] == model], model, host=False)
        check(mt, [q for q in sc.values() if q["camera"] == model], model, host=False, depth_is_positive=True, reproj_err_thr=2.0, parallax_deg_thr=3.0)


def test_optional_output_absent_and_two_calls_back_to_back(mt):
    import torch
    check(mt, [S.pose_problem(91, 120, "fisheye", n_slots=130, noise=5e-4)], "fisheye", skip_optional=True, host=False)
    p1, k1 = inputs([S.pose_problem(95, 300, "perspective", n_slots=320, noise=5e-4), S.pose_problem(96, 20, "perspective")], "perspective")
    p2, k2 = inputs([S.pose_problem(97, 64, "perspective", n_slots=70, noise=5e-4)], "perspective")
    o1, keep1 = enqueue_device(mt, p1, k1)
    o2, keep2 = enqueue_device(mt, p2, k2)                                        # reuses the context's buffers behind the first, nothing synchronised
    torch.cuda.synchronize()
    for pos, kw, o in ((p1, k1, o1), (p2, k2, o2)):
        want = plp.model_two_view_pose(*pos, out=sentinels(*pos[3].shape), **kw)
        for k in want:
            assert same_bits(o[k].cpu().numpy(), want[k]), k


def test_initializer_step_run_chains_both_entries_without_the_host(mt):
    import torch
    step_mod = importlib.import_module(plp.__name__ + ".initializer_step")
    model = "fisheye"
    qs = [S.pose_problem(61, 200, model, n_slots=220, noise=5e-4, mismatch=0.1), S.pose_problem(62, 40, model, mismatch=1.0), S.pose_problem(63, 5, model, n_slots=9)]
    a = S.pose_pack([dict(q, iters=8, samples=q["samples"][:8]) for q in qs])
    cam = plp.camera_model(S.CAMERAS[model])
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    kp = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda()
    step = step_mod.initializer_step(plp, mt=mt)
    r = step.run(cam, d(a["bearing_1"]), d(a["bearing_2"]), d(a["match"]), kp(a["undist_1"]), kp(a["undist_2"]), counts_1=d(a["counts_1"]), counts_2=d(a["counts_2"]),
                 seed=13, img_bounds=S.bounds(S.ref_camera(model)))
    torch.cuda.synchronize()
    e = plp.model_essential_ransac(a["bearing_1"], a["bearing_2"], a["match"], iters=100, seed=13, counts_1=a["counts_1"], counts_2=a["counts_2"], outputs=("inliers",))
    w = plp.model_two_view_pose(cam, e["E_21"], e["inliers"], a["match"], a["bearing_1"], a["bearing_2"], a["undist_1"], a["undist_2"], in_status=e["status"],
                                counts_1=a["counts_1"], counts_2=a["counts_2"], img_bounds=S.bounds(S.ref_camera(model)), outputs=())
    for k in w:
        assert same_bits(r[k].cpu().numpy(), w[k]), k
    assert same_bits(r["essential"]["E_21"].cpu().numpy(), e["E_21"]) and same_bits(r["essential"]["inliers"].cpu().numpy(), e["inliers"])
    assert w["status"].tolist() == [plp.TWO_VIEW_OK, plp.TWO_VIEW_NO_SOLUTION, plp.TWO_VIEW_NO_SOLUTION]


def test_argument_checks_of_both_entries(mt):
    import torch
    pos, kw = inputs([S.pose_problem(1, 12, "perspective")], "perspective")
    out = sentinels(1, 12)
    with pytest.raises(plp.PlpError) as ex:
        mt.two_view_pose(*pos, out=out, min_num_triangulated=-1, **kw)
    assert ex.value.status == plp.PLP_ERR_INVALID_ARG and all((v == SENT[v.dtype]).all() for v in out.values())
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(1, 12).items()}
    dev = [torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda() if v.dtype == plp.KP_DTYPE else d(v) for v in pos[1:]]
    m_cap = pos[5].shape[1]
    with pytest.raises(plp.PlpError) as ex:
        mt.two_view_pose_device(pos[0], 1, 12, m_cap, None, *dev[1:], o)
    assert ex.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as ex:
        mt.two_view_pose_device(pos[0], 1, 12, m_cap, *dev, {k: v for k, v in o.items() if k != "num_valid"})
    assert ex.value.status == plp.PLP_ERR_INVALID_ARG
    mt.two_view_pose_device(pos[0], 0, 12, m_cap, *dev, o)                          # nothing to do
    torch.cuda.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy() == SENT[np.dtype(plp.TWO_VIEW_OUTPUTS[k][1])]).all(), k
