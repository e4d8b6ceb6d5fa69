"""Local bundle adjustment of one new key frame's neighbourhood: map tables and the local key frames in, optimised poses and positions written back
into the tables and the outlier observations out, on one stream, without the host.

`local_ba_step.run` does what mapping_module runs for every new key frame (mapping_module.cc:251-261), optimize::local_bundle_adjuster::optimize
(optimize/local_bundle_adjuster.cc:62-410), on the tables landmark_refresh_step reads:

  1  plp_local_ba_device    the sets, both rounds and step [7]'s verdicts for the problem kf_local                                        :72-369
  2  torch, on the stream   local_keyfrm->set_cam_pose(...) and local_lm->set_pos_in_world(...) as row selections of static shape into the caller's
                            pose and pos_w tensors (:392-407); the outlier mask over the observation list                                 :345-369

With `lines`, the line tables of line_map_update_step, the step does what mapping_module runs when line tracking is on (mapping_module.cc:252-257),
optimize::local_bundle_adjuster_extended_line::optimize (optimize/local_bundle_adjuster_extended_line.cc:70-674):

  1  plp_local_ba_lines_device   the sets with the lines, both rounds over points and lines, step [7]'s verdicts of both kinds of edge          :108-573
  2  torch, on the stream        as above                                                                                                         :623-639
  3  line_map_update_step.run    mode TRIM_MAX_CHANGE with the adjuster's Pluecker estimates of the local lines: set_PlueckerCoord_without_update_endpoints,
                                 endpoint_trimming at the NEW poses, the end points or the erase flag, update_information                         :642-666

What stays on the host with lines is again step [8]'s map mutation: erase_landmark_line and erase_observation for every line outlier observation
(:606-615) and prepare_for_erasing for the lines whose skip_lines flag the update raised (:663).

No .item(), no copy to the host, no boolean-mask indexing.  What stays on the host is the map mutation of step [8]: keyfrm->erase_landmark(lm) and
lm->erase_observation(keyfrm) for every outlier observation (:382-388), with the choice of a new ref_keyfrm_ that erase_observation makes -- the
caller applies the mask to its observations_ maps, flattens them again and then runs landmark_refresh_step, which is update_normal_and_depth (:407)
for every landmark the adjuster moved.

Tables are torch tensors on the step's device, named as landmark_refresh_step names them:
  key frames  kps [F, cap, 28] u8 (undist_keypts_ as plp_keypoint), counts [F] i32 or absent, pose [F, 15] f64 (frame_pose rows; updated in place),
              kf_erased [F] u8, and for this step x_right [F, cap] f32 (stereo_x_right_; absent = monocular), kf_is_origin [F] u8 (id_ == 0; absent = none)
  landmarks   pos_w [L, 3] f64 (updated in place), skip [L] u8 or absent (will_be_erased()), obs_offsets [L + 1] i32, obs_kf / obs_idx [T] i32
  kf_local    [F] u8: the current key frame and the covisibilities the caller chose (:73-91)
  lines       line_map_update_step's line tables (pluecker_lines, pos_w_lines, ref_kf_lines, skip_lines, obs_offsets_lines, obs_kf_lines, obs_idx_lines, ...), with
              the key frames' kl [F, lcap, 68] u8, kl_counts and what TRIM_MAX_CHANGE needs: median_depth [F] f32, or kf_lm [F, cap] i32
"""
import numpy as np


class local_ba_step:
    def __init__(self, plp, camera, setup_type, inv_level_sigma_sq, num_first_iter=5, num_second_iter=10, device_index=0, mt=None, inv_level_sigma_sq_lsd=None,
                 line_update=None):
        """camera: a plp.camera_model; setup_type 0 monocular, 1 stereo, 2 RGB-D; inv_level_sigma_sq: the key frames' inv_level_sigma_sq_ (host,
        num_levels floats); the iteration counts are the adjuster's defaults.  For run(lines=): inv_level_sigma_sq_lsd, the key frames'
        _inv_level_sigma_sq_lsd, and line_update, a line_map_update_step (default: one over the same matcher)"""
        import torch
        self.torch, self.plp, self.camera, self.setup_type = torch, plp, camera, int(setup_type)
        self.dev = torch.device("cuda", device_index)
        self.sigma = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
        self.num_first_iter, self.num_second_iter = int(num_first_iter), int(num_second_iter)
        self.mt = mt or plp.matcher(device=device_index)
        self.sigma_lsd = None if inv_level_sigma_sq_lsd is None else np.ascontiguousarray(inv_level_sigma_sq_lsd, np.float32).reshape(-1)
        self.line_update, self.device_index = line_update, device_index

    def run(self, keyframes, landmarks, kf_local, lines=None, stream=None):
        """Enqueue the steps on `stream` (default: the current stream).  keyframes["pose"] and landmarks["pos_w"] are rewritten where the adjuster
        writes them.  Returns dict(the outputs of plp_local_ba_device named as in LOCAL_BA_OUTPUTS, each with a leading 1, and outlier_mask [T] u8:
        the observations step [8] erases).  With lines: the adjuster with line landmarks runs instead, the line tables are updated by
        line_map_update_step.run, and the dict also holds LOCAL_BA_LINES_OUTPUTS, outlier_mask_lines [TL] u8 and line_update, that run's dict.
        Nothing is synchronised."""
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
        if lines is not None:
            return self._run_lines(keyframes, landmarks, local, lines, out, st)
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

    def _run_lines(self, keyframes, landmarks, local, lines, out, st):
        torch, plp = self.torch, self.plp
        if self.sigma_lsd is None:
            raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, "run(lines=) needs the step's inv_level_sigma_sq_lsd")
        if self.line_update is None:
            import importlib
            mod = importlib.import_module(__package__ + ".line_map_update_step")
            self.line_update = mod.line_map_update_step(plp, self.camera, device_index=self.device_index, mt=self.mt)
        pose, pos_w, kl, pk = keyframes["pose"], landmarks["pos_w"], keyframes["kl"], lines["pluecker_lines"]
        F, L, T, cap = pose.shape[0], pos_w.shape[0], landmarks["obs_kf"].shape[0], keyframes["kps"].shape[1]
        LL, TL = pk.shape[0], lines["obs_kf_lines"].shape[0]
        tt = {np.uint8: torch.uint8, np.float64: torch.float64}
        with torch.cuda.stream(st):
            out.update({k: torch.zeros((1,) + shape(LL, TL), dtype=tt[dt], device=self.dev) for k, (shape, dt) in plp.LOCAL_BA_LINES_OUTPUTS.items()})
        self.mt.local_ba_lines_device(self.camera, self.setup_type, 1, F, L, T, cap, pose, keyframes["kps"], pos_w, landmarks["obs_offsets"], landmarks["obs_kf"],
                                      landmarks["obs_idx"], local, self.sigma, LL, TL, kl.shape[1], kl, pk, lines["obs_offsets_lines"], lines["obs_kf_lines"],
                                      lines["obs_idx_lines"], self.sigma_lsd, {k: v for k, v in out.items() if v.numel()}, x_right=keyframes.get("x_right"),
                                      counts=keyframes.get("counts"), kf_erased=keyframes.get("kf_erased"), kf_is_origin=keyframes.get("kf_is_origin"),
                                      lm_erased=landmarks.get("skip"), kl_counts=keyframes.get("kl_counts"), line_erased=lines.get("skip_lines"),
                                      pose_stride=pose.shape[1], num_first_iter=self.num_first_iter, num_second_iter=self.num_second_iter, stream=st)
        with torch.cuda.stream(st):
            ok = out["status"][0] == plp.LOCAL_BA_OK
            free = (out["kf_role"][0] == plp.LOCAL_BA_KF_FREE) & ok
            moved = (out["lm_role"][0] == 1) & ok
            pose[:, :15].copy_(torch.where(free.unsqueeze(1), out["pose"][0], pose[:, :15]))
            pos_w.copy_(torch.where(moved.unsqueeze(1), out["pos_w"][0], pos_w))
            out["outlier_mask"] = (out["outlier"][0] == 1).to(torch.uint8)
            out["outlier_mask_lines"] = (out["outlier_lines"][0] == 1).to(torch.uint8)
            moved_lines = ((out["line_role"][0] == 1) & ok).to(torch.uint8)
        median = keyframes.get("median_depth")
        out["line_update"] = self.line_update.run(keyframes, lines, mode=plp.TRIM_MAX_CHANGE, pluecker=out["pluecker"][0], moved=moved_lines, median_depth=median,
                                                  points_pos_w=None if median is not None else pos_w, stream=st)
        return out
