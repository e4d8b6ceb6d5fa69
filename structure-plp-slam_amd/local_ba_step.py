"""Local bundle adjustment of one new key frame's neighbourhood: map tables and the local key frames in, optimised poses and positions written back
into the tables and the outlier observations out, on one stream, without the host.

`local_ba_step.run` does what mapping_module runs for every new key frame (mapping_module.cc:251-261), optimize::local_bundle_adjuster::optimize
(optimize/local_bundle_adjuster.cc:62-410), on the tables landmark_refresh_step reads:

  1  plp_local_ba_device    the sets, both rounds and step [7]'s verdicts for the problem kf_local                                        :72-369
  2  torch, on the stream   local_keyfrm->set_cam_pose(...) and local_lm->set_pos_in_world(...) as row selections of static shape into the caller's
                            pose and pos_w tensors (:392-407); the outlier mask over the observation list                                 :345-369

No .item(), no copy to the host, no boolean-mask indexing.  What stays on the host is the map mutation of step [8]: keyfrm->erase_landmark(lm) and
lm->erase_observation(keyfrm) for every outlier observation (:382-388), with the choice of a new ref_keyfrm_ that erase_observation makes -- the
caller applies the mask to its observations_ maps, flattens them again and then runs landmark_refresh_step, which is update_normal_and_depth (:407)
for every landmark the adjuster moved.

Tables are torch tensors on the step's device, named as landmark_refresh_step names them:
  key frames  kps [F, cap, 28] u8 (undist_keypts_ as plp_keypoint), counts [F] i32 or absent, pose [F, 15] f64 (frame_pose rows; updated in place),
              kf_erased [F] u8, and for this step x_right [F, cap] f32 (stereo_x_right_; absent = monocular), kf_is_origin [F] u8 (id_ == 0; absent = none)
  landmarks   pos_w [L, 3] f64 (updated in place), skip [L] u8 or absent (will_be_erased()), obs_offsets [L + 1] i32, obs_kf / obs_idx [T] i32
  kf_local    [F] u8: the current key frame and the covisibilities the caller chose (:73-91)
"""
import numpy as np


class local_ba_step:
    def __init__(self, plp, camera, setup_type, inv_level_sigma_sq, num_first_iter=5, num_second_iter=10, device_index=0, mt=None):
        """camera: a plp.camera_model; setup_type 0 monocular, 1 stereo, 2 RGB-D; inv_level_sigma_sq: the key frames' inv_level_sigma_sq_ (host,
        num_levels floats); the iteration counts are the adjuster's defaults"""
        import torch
        self.torch, self.plp, self.camera, self.setup_type = torch, plp, camera, int(setup_type)
        self.dev = torch.device("cuda", device_index)
        self.sigma = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
        self.num_first_iter, self.num_second_iter = int(num_first_iter), int(num_second_iter)
        self.mt = mt or plp.matcher(device=device_index)

    def run(self, keyframes, landmarks, kf_local, stream=None):
        """Enqueue both steps on `stream` (default: the current stream).  keyframes["pose"] and landmarks["pos_w"] are rewritten where the adjuster
        writes them.  Returns dict(the outputs of plp_local_ba_device named as in LOCAL_BA_OUTPUTS, each with a leading 1, and outlier_mask [T] u8:
        the observations step [8] erases).  Nothing is synchronised."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        pose, pos_w = keyframes["pose"], landmarks["pos_w"]
        F, L, T, cap = pose.shape[0], pos_w.shape[0], landmarks["obs_kf"].shape[0], keyframes["kps"].shape[1]
        if not (pose.is_contiguous() and pos_w.is_contiguous()):
            raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, "pose and pos_w must be contiguous: they are updated in place")
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
        with torch.cuda.stream(st):
            out = {k: torch.zeros((1,) + shape(F, L, T), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in plp.LOCAL_BA_OUTPUTS.items()}
            local = kf_local.reshape(1, F).to(torch.uint8).contiguous()
        self.mt.local_ba_device(self.camera, self.setup_type, 1, F, L, T, cap, pose, keyframes["kps"], pos_w, landmarks["obs_offsets"], landmarks["obs_kf"],
                                landmarks["obs_idx"], local, self.sigma, {k: v for k, v in out.items() if v.numel()}, x_right=keyframes.get("x_right"),
                                counts=keyframes.get("counts"), kf_erased=keyframes.get("kf_erased"), kf_is_origin=keyframes.get("kf_is_origin"),
                                lm_erased=landmarks.get("skip"), pose_stride=pose.shape[1], num_first_iter=self.num_first_iter,
                                num_second_iter=self.num_second_iter, stream=st)
        with torch.cuda.stream(st):
            ok = out["status"][0] == plp.LOCAL_BA_OK
            free = (out["kf_role"][0] == plp.LOCAL_BA_KF_FREE) & ok
            moved = (out["lm_role"][0] == 1) & ok
            pose[:, :15].copy_(torch.where(free.unsqueeze(1), out["pose"][0], pose[:, :15]))
            pos_w.copy_(torch.where(moved.unsqueeze(1), out["pos_w"][0], pos_w))
            out["outlier_mask"] = (out["outlier"][0] == 1).to(torch.uint8)
        return out
