"""perspective::reconstruct_with_H / reconstruct_with_F on the device (plp_perspective_pose_device / _host, csrc/perspective_pose_kernels.hip) against
the CPU build of the same header (plp.model_perspective_pose, which tests/test_perspective_init_cpu.py holds bit for bit to the restatement; DESIGN.md
section 5, D27 items e and h): every output bit for bit on sentinel-filled arrays -- perspective and fisheye cameras, H problems (eight hypotheses)
and F problems (four) in one call with every status, inlier counts around the order-statistic index (50 / 51 / 52) and the 256 slots of a pass
(256 / 257), the choice, matrices and mask taken from the RANSAC entry on one stream without synchronisation, the equirectangular camera refused
with nothing written, and the slots above counts_1 untouched."""
import numpy as np
import pytest

import perspective_init_scene as S
import two_view_scene as TS
from plp import plp
from test_gpu_perspective_ransac import SENT, same_bits, to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap):
    return {k: np.full((P,) + shape(n_cap), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.PERSPECTIVE_POSE_OUTPUTS.items()}


def pack_pose(problems):
    """S.pack plus the bearings; slots and key points above a problem's own hold values the counts hide"""
    a = S.pack(problems)
    P, n_cap, m_cap = len(problems), a["match"].shape[1], a["undist_2"].shape[1]
    a["bearing_1"], a["bearing_2"] = np.full((P, n_cap, 3), 0.5), np.full((P, m_cap, 3), 0.5)
    for p, q in enumerate(problems):
        a["bearing_1"][p, :len(q["bearing_1"])], a["bearing_2"][p, :len(q["bearing_2"])] = q["bearing_1"], q["bearing_2"]
    return a


def rotation_homography(q):
    c = TS.ref_camera(q["camera"])
    K = np.array([[c["fx"], 0.0, c["cx"]], [0.0, c["fy"], c["cy"]], [0.0, 0.0, 1.0]])
    return K @ q["truth"][0] @ np.linalg.inv(K)


def check(mt, problems, camera="perspective", force=None, host=True, **kw):
    """RANSAC (host build) -> pose: device entry on the RANSAC entry's own device outputs, host entry and host build.  force: {p: (choice, H)}"""
    import torch
    from test_gpu_perspective_ransac import enqueue_device
    a = pack_pose(problems)
    P, n_cap = a["match"].shape
    m_cap = a["undist_2"].shape[1]
    cam = plp.camera_model(TS.CAMERAS[camera])
    bounds = problems[0]["bounds"]
    ra = {k: a[k] for k in ("undist_1", "undist_2", "match", "samples_h", "samples_f", "counts_1", "counts_2")}
    pos, rkw = S.call_kwargs(ra)
    e = plp.model_perspective_ransac(*pos, **rkw)
    o, dev = enqueue_device(mt, ra, True, None)                      # the RANSAC on the device; nothing is synchronised before the pose entry
    if force:
        torch.cuda.synchronize()
        for p, (choice, Hm) in force.items():
            e["choice"][p], e["H_21"][p] = choice, Hm
        o["choice"], o["H_21"] = to_device(e["choice"]), to_device(e["H_21"])
    want = plp.model_perspective_pose(cam, e["choice"], e["H_21"], e["F_21"], e["inliers"], a["match"], a["bearing_1"], a["bearing_2"], a["undist_1"], a["undist_2"],
                                      counts_1=a["counts_1"], counts_2=a["counts_2"], img_bounds=bounds, out=sentinels(P, n_cap), **kw)
    for p in range(P):
        assert (want["is_triangulated"][p, int(a["counts_1"][p]):] == SENT[np.dtype(np.uint8)]).all()
    d = {k: to_device(v) for k, v in sentinels(P, n_cap).items()}
    mt.perspective_pose_device(cam, P, n_cap, m_cap, o["choice"], o["H_21"], o["F_21"], o["inliers"], dev["match"], to_device(a["bearing_1"]), to_device(a["bearing_2"]),
                               dev["undist_1"], dev["undist_2"], d, counts_1=dev["counts_1"], counts_2=dev["counts_2"], img_bounds=bounds, **kw)
    torch.cuda.synchronize()
    for k in want:
        assert same_bits(d[k].cpu().numpy(), want[k]), ("device", k, d[k].cpu().numpy(), want[k])
    if host:
        h = mt.perspective_pose(cam, e["choice"], e["H_21"], e["F_21"], e["inliers"], a["match"], a["bearing_1"], a["bearing_2"], a["undist_1"], a["undist_2"],
                                counts_1=a["counts_1"], counts_2=a["counts_2"], img_bounds=bounds, out=sentinels(P, n_cap), **kw)
        for k in want:
            assert same_bits(h[k], want[k]), ("host entry", k)
    return e, want


def test_h_and_f_problems_with_every_status_in_one_call(mt):
    qs = [S.problem(510, 150, "perspective", n_slots=160, noise=5e-4, mismatch=0.1, kind="planar"), S.problem(502, 200, "perspective", n_slots=214, noise=3e-4, mismatch=0.15),
          S.problem(500, 150, "perspective", n_slots=160, noise=5e-4, mismatch=0.1, kind="planar"), S.problem(501, 64, "perspective", n_slots=71, noise=1e-3, mismatch=0.2),
          S.problem(504, 120, "perspective", n_slots=130, noise=5e-4, mismatch=0.1, kind="near_rotation"), S.problem(507, 60, "perspective", mismatch=1.0),
          S.problem(508, 7, "perspective", n_slots=12), S.problem(513, 150, "perspective", n_slots=160, noise=5e-4, mismatch=0.1, kind="planar")]
    e, w = check(mt, qs, force={7: (plp.PERSPECTIVE_CHOICE_H, rotation_homography(qs[7]))})
    assert set(w["status"].tolist()) == {plp.TWO_VIEW_OK, plp.TWO_VIEW_NO_SOLUTION, plp.TWO_VIEW_TOO_FEW_TRIANGULATED, plp.TWO_VIEW_AMBIGUOUS,
                                         plp.TWO_VIEW_SMALL_PARALLAX, plp.PERSPECTIVE_POSE_NO_DECOMPOSITION}, w["status"]
    assert w["status"][0] == w["status"][1] == plp.TWO_VIEW_OK and e["choice"][0] == plp.PERSPECTIVE_CHOICE_H and e["choice"][1] == plp.PERSPECTIVE_CHOICE_F
    assert w["status"][7] == plp.PERSPECTIVE_POSE_NO_DECOMPOSITION and not w["num_valid"][7].any()
    assert (w["num_valid"][0] > 0).sum() > 1 and not w["num_valid"][1][4:].any()


def test_fisheye_camera(mt):
    qs = [S.problem(503, 200, "fisheye", n_slots=207, noise=2e-3, mismatch=0.2, iters=12), S.problem(520, 150, "fisheye", n_slots=160, noise=5e-4, kind="planar", iters=12)]
    e, w = check(mt, qs, camera="fisheye", min_num_triangulated=20)
    assert w["status"][0] == plp.TWO_VIEW_OK


@pytest.mark.parametrize("n_in", [50, 51, 52, 255, 256, 257])
def test_inlier_counts_around_the_order_statistic_and_the_pass(mt, n_in):
    """exact matches only: every match is an inlier of both solvers and, but for a few whose point leaves the image, valid under the true pose: in each
    case one of the two problems' lists of cos_parallaxes holds exactly n_in keys (the other a few less), on both sides of index 50 and of the 256 of a pass"""
    qs = [S.problem(800 + n_in, n_in, "perspective", n_slots=n_in + 9, noise=0.0, iters=6), S.problem(900 + n_in, n_in, "perspective", n_slots=n_in + 3, noise=0.0, iters=6,
                                                                                                       kind="planar")]
    e, w = check(mt, qs, host=False, min_num_triangulated=10)
    assert w["num_valid"].max() == n_in


def test_the_equirectangular_camera_is_refused_with_nothing_written(mt):
    q = S.problem(501, 64, "perspective", n_slots=71)
    a = pack_pose([q])
    out = sentinels(1, a["match"].shape[1])
    with pytest.raises(plp.PlpError) as err:
        mt.perspective_pose(plp.camera_model(TS.CAMERAS["equirectangular"]), [2], np.eye(3)[None], np.eye(3)[None], np.ones_like(a["match"], np.uint8), a["match"],
                            a["bearing_1"], a["bearing_2"], a["undist_1"], a["undist_2"], img_bounds=q["bounds"], out=out)
    assert err.value.status == plp.PLP_ERR_UNSUPPORTED and all((v == SENT[v.dtype]).all() for v in out.values())
