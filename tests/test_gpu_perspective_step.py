"""initializer_step.run_perspective -- plp_perspective_ransac_device -> plp_perspective_pose_device on tensors that stay on the device (DESIGN.md
section 5, D27) -- against the perspective_initializer mirror class on the host builds, problem by problem, and a planar and a cloud scene against
their ground truth (the bound of tests/test_perspective_init_cpu.py: twice the error of an independent fit)."""
import importlib

import numpy as np
import pytest

import perspective_init_scene as S
import two_view_scene as TS
from plp import plp
from test_gpu_perspective_pose import pack_pose
from test_gpu_perspective_ransac import same_bits, to_device

pytestmark = pytest.mark.gpu


def test_run_perspective_equals_the_mirror_class_problem_by_problem_and_recovers_the_scenes_motion():
    import torch
    from test_perspective_init_cpu import angle_dir, angle_rot, independent_pose_error
    step_mod = importlib.import_module(plp.__name__ + ".initializer_step")
    names = ["planar_pose", "cloud_200", "all_mismatched", "seven"]
    qs = [S.problem(510, 150, "perspective", n_slots=160, noise=5e-4, mismatch=0.1, kind="planar"), S.problem(502, 200, "perspective", n_slots=214, noise=3e-4, mismatch=0.15),
          S.problem(507, 60, "perspective", mismatch=1.0), S.problem(508, 7, "perspective", n_slots=12)]
    a = pack_pose(qs)
    cam = plp.camera_model(TS.CAMERAS["perspective"])
    step = step_mod.initializer_step(plp, num_ransac_iters=24)
    d = {k: to_device(v) for k, v in a.items()}
    out = step.run_perspective(cam, d["bearing_1"], d["bearing_2"], d["match"], d["undist_1"], d["undist_2"], counts_1=d["counts_1"], counts_2=d["counts_2"],
                               samples_h=d["samples_h"], samples_f=d["samples_f"], img_bounds=qs[0]["bounds"])
    torch.cuda.synchronize()
    for p, q in enumerate(qs):
        init = plp.perspective_initializer(cam, q["undist_1"], q["bearing_1"], num_ransac_iters=24, samples_h=q["samples_h"][None], samples_f=q["samples_f"][None])
        ok = init.initialize(q["undist_2"], q["bearing_2"], q["match"])
        n = len(q["match"])
        assert ok == (int(out["status"][p]) == plp.TWO_VIEW_OK) == (p < 2), names[p]
        assert same_bits(out["rot_ref_to_cur"][p].cpu().numpy(), init.get_rotation_ref_to_cur()) and same_bits(out["trans_ref_to_cur"][p].cpu().numpy(), init.get_translation_ref_to_cur())
        assert same_bits(out["triangulated_pts"][p, :n].cpu().numpy(), init.get_triangulated_pts()) and out["is_triangulated"][p, :n].cpu().numpy().astype(bool).tolist() == init.get_triangulated_flags().tolist()
        assert int(out["ransac"]["choice"][p]) == int(init.ransac["choice"][0]) == (plp.PERSPECTIVE_CHOICE_H, plp.PERSPECTIVE_CHOICE_F, 0, 0)[p]
        if p < 2:
            Rt, tt = q["truth"]
            rot_i, tr_i = independent_pose_error(q, names[p])
            assert angle_rot(out["rot_ref_to_cur"][p].cpu().numpy(), Rt) <= max(2 * rot_i, 1e-6) and angle_dir(out["trans_ref_to_cur"][p].cpu().numpy(), tt) <= max(2 * tr_i, 1e-5)
