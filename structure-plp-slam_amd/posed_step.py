"""The tracker's four per-frame matcher calls from real geometry: poses and landmarks in, matches out, on one stream, without the host.

For B frames whose features are already in HBM (extractor outputs plus the post-extract `undist`, `x_right` and key-line `x_right` pairs),
`posed_tracker_step.run` does what module/frame_tracker.cc:66-87 (motion_based_track) and tracking_module.cc:908-1064
(search_local_landmarks[_line]) do per frame:

  1  plp_project_last_frame_device        -> PLP_MATCH_MODE_LAST_FRAME        match_current_and_last_frames       pose_pred, directions from 1
  2  plp_project_last_frame_lines_device  -> PLP_MATCH_MODE_LAST_FRAME_LINE   match_current_and_last_frames_line  pose_pred, directions from 2
  3  plp_observe_landmarks_device         -> PLP_MATCH_MODE_LANDMARKS         match_frame_and_landmarks           pose
  4  plp_observe_landmark_lines_device    -> PLP_MATCH_MODE_LANDMARKS_LINE    match_frame_and_landmarks_line      pose

The projections write their outputs in the layout the matcher reads, so nothing is copied between a projection and its matcher.  The
current frame's `landmarks_` are cleared before call 1 (frame_tracker.cc:61): calls 1 and 2 see no occupied key point.  Calls 3 and 4 see
the key points / key lines the last-frame calls matched to a landmark with an observation (what `landmarks_[idx] && has_observation()` reads
there) unless the caller passes its own arrays (e.g. after removing the pose optimiser's outliers).  Pose optimisation lives in
pose_optimization_step.py (tracked_pose_step: run_last_frame, plp_pose_optimize_device, run_local, plp_pose_optimize_device again); the widened
second search of motion_based_track and the host's writes back to the landmark objects are not part of the step.

Tables are torch tensors on the step's device, one row per frame:
  frame  kps [B, cap, 28] u8 (undist_keypts_ as plp_keypoint), desc [B, cap, 32], counts [B], x_right [B, cap] f32 or None,
         kl [B, lcap, 68] u8 (_keylsd as plp_keyline), lbd [B, lcap, 32], kl_counts [B], kl_x_right [B, lcap, 2] f32 or None
  last   pose [B, 15] f64 (frame_pose of the last frame); points: pos_w [B, m, 3] f64, skip [B, m] u8 ("!landmarks_[j] || outlier_flags_[j]"),
         counts [B], keypts [B, m, 28] u8 (its undist_keypts_), desc [B, m, 32] (lm->get_descriptor()), has_obs [B, m] u8;
         lines: the same keys with the suffix _lines (pos_w_lines [B, ml, 6], keylines_lines [B, ml, 68] u8 = its _keylsd, ...)
  local  points: pos_w [B, L, 3] f64, normal [B, L, 3] f64, min_dist / max_dist [B, L] f32, skip [B, L] u8, counts [B], desc [B, L, 32],
         has_obs [B, L] u8; lines: pos_w_lines [B, LL, 6], min_dist_lines, max_dist_lines, skip_lines, counts_lines, desc_lines, has_obs_lines
"""
import math

import numpy as np


class posed_tracker_step:
    def __init__(self, plp, camera, setup_type, true_baseline=0.0, scale_factor=1.2, num_levels=8, scale_factor_lsd=2.0, num_levels_lsd=1,
                 margin_last=None, margin_last_line=20.0, margin_local=None, margin_local_line=10.0, device_index=0):
        """camera: a plp.camera_model; setup_type: plp.SETUP_MONOCULAR / SETUP_STEREO / SETUP_RGBD.  Margins default to the reference's for a
        frame that is not right after a relocalisation: 20 (10 for stereo) for the last frame, 20 for its lines (frame_tracker.cc:64, 84),
        10 for RGB-D and 5 otherwise for local landmarks, 10 for local lines (tracking_module.cc:978-982, 1057-1059)."""
        import torch
        self.torch, self.plp, self.camera = torch, plp, camera
        self.dev = torch.device("cuda", device_index)
        self.setup_type, self.true_baseline = int(setup_type), float(true_baseline)
        stereo, rgbd = self.setup_type == plp.SETUP_STEREO, self.setup_type == plp.SETUP_RGBD
        self.margin_last = float(margin_last if margin_last is not None else (10.0 if stereo else 20.0))
        self.margin_last_line = float(margin_last_line)
        self.margin_local = float(margin_local if margin_local is not None else (10.0 if rgbd else 5.0))
        self.margin_local_line = float(margin_local_line)
        f32 = np.float32
        self.sf = np.ones(num_levels, np.float32)                     # orb_params::calc_scale_factors: float products
        for i in range(1, num_levels):
            self.sf[i] = f32(self.sf[i - 1] * f32(scale_factor))
        self.sf_lsd = np.ones(num_levels_lsd, np.float32)
        for i in range(1, num_levels_lsd):
            self.sf_lsd[i] = f32(self.sf_lsd[i - 1] * f32(scale_factor_lsd))
        self.log_sf = f32(math.log(f32(scale_factor)))                 # frame::log_scale_factor_ (logf as D5 defines it)
        self.log_sf_lsd = f32(math.log(f32(scale_factor_lsd)))
        self.num_levels, self.num_levels_lsd = int(num_levels), int(num_levels_lsd)
        self.grid = camera.grid()
        # match::projection(0.9, true) in motion_based_track, projection(0.8) (orientation check on by default) in search_local_landmarks[_line]
        self.mt_last = plp.matcher(0.9, True, device=device_index)
        self.mt_last_line = plp.matcher(0.9, True, device=device_index)
        self.mt_local = plp.matcher(0.8, True, device=device_index)
        self.mt_local_line = plp.matcher(0.8, True, device=device_index)
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def run(self, frame, last, local, pose_pred, pose=None, t_occupied=None, t_occupied_lines=None, stream=None):
        """Enqueue the four calls for the B frames on `stream` (default: the current stream).  pose_pred / pose: [B, 15] f64 (frame_pose rows);
        pose None = pose_pred.  t_occupied [B, cap] / t_occupied_lines [B, lcap] u8: the occupancy calls 3 / 4 see, None = what calls 1 / 2 left.
        Returns dict(m1, n1, m2, n2, m3, n3, m4, n4): out_match [B, n_cap] / out_num [B] of the four calls (LAST_FRAME, LANDMARKS, LAST_FRAME_LINE,
        LANDMARKS_LINE), and the intermediate query arrays under q1 ... q4.  Nothing is synchronised; the returned tensors are the step's own
        buffers, rewritten by the next run."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        out = self.run_last_frame(frame, last, pose_pred, stream=st)
        # what calls 3 and 4 see as occupied: curr_frm.landmarks_[idx] && has_observation() after the last-frame calls
        with torch.cuda.stream(st):
            if t_occupied is None:
                t_occupied = self._occupied(out["m1"], frame["counts"], last.get("has_obs"))
            if t_occupied_lines is None:
                t_occupied_lines = self._occupied(out["m3"], frame["kl_counts"], last.get("has_obs_lines"))
        out.update(self.run_local(frame, local, pose_pred if pose is None else pose, t_occupied, t_occupied_lines, stream=st))
        return out

    def _targets(self, frame, st, last_frame=True):
        torch = self.torch
        t = dict(t_kps=frame["kps"], t_desc=frame["desc"], t_counts=frame["counts"], t_x_right=frame.get("x_right"))
        kxr = frame.get("kl_x_right")
        tl = dict(t_kl=frame["kl"], t_desc=frame["lbd"], t_counts=frame["kl_counts"])
        tl_last = dict(tl)
        if kxr is not None and last_frame:   # _stereo_x_right_cooresponding_to_keylines first / second as the two arrays LAST_FRAME_LINE's RGB-D gate reads
            with torch.cuda.stream(st):
                tl_last["t_x_right"], tl_last["t_x_right2"] = kxr[..., 0].contiguous(), kxr[..., 1].contiguous()
        return t, tl, tl_last

    def run_last_frame(self, frame, last, pose_pred, stream=None):
        """Calls 1 and 2 of run() alone (a pose optimiser may sit between them and calls 3 and 4: pose_optimization_step.py): dict(m1, n1, q1,
        direction, m3, n3, q3, direction_lines)."""
        torch, plp, cam = self.torch, self.plp, self.camera
        st = stream or torch.cuda.current_stream(self.dev)
        B, cap = frame["kps"].shape[0], frame["kps"].shape[1]
        lcap = frame["kl"].shape[1]
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        t, tl, tl_last = self._targets(frame, st)
        rgbd = self.setup_type == plp.SETUP_RGBD
        out = {}

        # 1  last frame, points
        m = last["pos_w"].shape[1]
        q1 = dict(q_reproj=self._buf("q1_reproj", (B, m, 2), f32), q_x_right=self._buf("q1_xr", (B, m), f32), q_level=self._buf("q1_level", (B, m), i32),
                  q_angle=self._buf("q1_angle", (B, m), f32), q_valid=self._buf("q1_valid", (B, m), u8))
        d1 = self._buf("dir1", (B,), i32)
        self.mt_last.project_last_frame_device(cam, B, m, pose_pred, last["pose"], last["pos_w"], last["keypts"], q1["q_reproj"], q1["q_level"], q1["q_valid"], d1,
                                               skip=last.get("skip"), counts=last.get("counts"), out_x_right=q1["q_x_right"], out_angle=q1["q_angle"],
                                               setup_type=self.setup_type, true_baseline=self.true_baseline, stream=st)
        q1.update(q_desc=last["desc"], q_has_obs=last.get("has_obs"), q_counts=last.get("counts"))
        m1, n1 = self._buf("m1", (B, cap), i32), self._buf("n1", (B,), i32)
        self.mt_last.match_device(plp.MODE_LAST_FRAME, cap, m, {**t, **q1}, m1, n1, margin=self.margin_last, scale_factors=self.sf, grid=self.grid, B=B,
                                  stream=st, directions=d1)
        out.update(m1=m1, n1=n1, q1=q1, direction=d1)

        # 2  last frame, lines
        ml = last["pos_w_lines"].shape[1]
        q3 = dict(q_reproj=self._buf("q3_sp", (B, ml, 2), f32), q_reproj2=self._buf("q3_ep", (B, ml, 2), f32), q_x_right=self._buf("q3_xs", (B, ml), f32),
                  q_x_right2=self._buf("q3_xe", (B, ml), f32), q_level=self._buf("q3_level", (B, ml), i32), q_valid=self._buf("q3_valid", (B, ml), u8))
        d3 = self._buf("dir3", (B,), i32)
        self.mt_last_line.project_last_frame_lines_device(cam, B, ml, pose_pred, last["pose"], last["pos_w_lines"], last["keylines_lines"], q3["q_reproj"],
                                                          q3["q_reproj2"], q3["q_level"], q3["q_valid"], d3, skip=last.get("skip_lines"),
                                                          counts=last.get("counts_lines"), out_x_right_sp=q3["q_x_right"], out_x_right_ep=q3["q_x_right2"],
                                                          setup_type=self.setup_type, true_baseline=self.true_baseline, stream=st)
        q3.update(q_desc=last["desc_lines"], q_has_obs=last.get("has_obs_lines"), q_counts=last.get("counts_lines"), is_rgbd=int(rgbd),
                  num_levels_lsd=self.num_levels_lsd)
        m3, n3 = self._buf("m3", (B, lcap), i32), self._buf("n3", (B,), i32)
        self.mt_last_line.match_device(plp.MODE_LAST_FRAME_LINE, lcap, ml, {**tl_last, **q3}, m3, n3, margin=self.margin_last_line, scale_factors=self.sf_lsd,
                                       B=B, stream=st, directions=d3)
        out.update(m3=m3, n3=n3, q3=q3, direction_lines=d3)

        return out

    def run_local(self, frame, local, pose, t_occupied, t_occupied_lines, stream=None):
        """Calls 3 and 4 of run() alone, with the occupancy they see given: dict(m2, n2, q2, t_occupied, m4, n4, q4, t_occupied_lines)."""
        torch, plp, cam = self.torch, self.plp, self.camera
        st = stream or torch.cuda.current_stream(self.dev)
        B, cap = frame["kps"].shape[0], frame["kps"].shape[1]
        lcap = frame["kl"].shape[1]
        i32, f32, u8 = torch.int32, torch.float32, torch.uint8
        t, tl, _ = self._targets(frame, st, False)
        out = {}

        # 3  local landmarks, points
        L = local["pos_w"].shape[1]
        q2 = dict(q_reproj=self._buf("q2_reproj", (B, L, 2), f32), q_x_right=self._buf("q2_xr", (B, L), f32), q_level=self._buf("q2_level", (B, L), i32),
                  q_valid=self._buf("q2_valid", (B, L), u8))
        self.mt_local.observe_landmarks_device(cam, B, L, pose, local["pos_w"], q2["q_reproj"], q2["q_valid"], obs_mean_normal=local["normal"],
                                               min_valid_dist=local["min_dist"], max_valid_dist=local["max_dist"], skip=local.get("skip"),
                                               counts=local.get("counts"), out_x_right=q2["q_x_right"], out_level=q2["q_level"],
                                               log_scale_factor=self.log_sf, num_levels=self.num_levels, stream=st)
        q2.update(q_desc=local["desc"], q_has_obs=local.get("has_obs"), q_counts=local.get("counts"))
        m2, n2 = self._buf("m2", (B, cap), i32), self._buf("n2", (B,), i32)
        self.mt_local.match_device(plp.MODE_LANDMARKS, cap, L, {**t, **q2, "t_occupied": t_occupied}, m2, n2, margin=self.margin_local, scale_factors=self.sf,
                                   grid=self.grid, B=B, stream=st)
        out.update(m2=m2, n2=n2, q2=q2, t_occupied=t_occupied)

        # 4  local landmarks, lines
        LL = local["pos_w_lines"].shape[1]
        q4 = dict(q_reproj=self._buf("q4_sp", (B, LL, 2), f32), q_reproj2=self._buf("q4_ep", (B, LL, 2), f32), q_level=self._buf("q4_level", (B, LL), i32),
                  q_valid=self._buf("q4_valid", (B, LL), u8))
        self.mt_local_line.observe_landmark_lines_device(cam, B, LL, pose, local["pos_w_lines"], local["min_dist_lines"], local["max_dist_lines"], q4["q_reproj"],
                                                         q4["q_reproj2"], q4["q_level"], q4["q_valid"], skip=local.get("skip_lines"),
                                                         counts=local.get("counts_lines"), log_scale_factor=self.log_sf_lsd, num_levels=self.num_levels_lsd,
                                                         stream=st)
        with torch.cuda.stream(st):   # undist_keypts_.at(idx).octave read with a key LINE index (projection.cc:187,192)
            kp_oct = frame["kps"].view(torch.int32)[:, :lcap, 5]
            if kp_oct.shape[1] < lcap:
                kp_oct = torch.nn.functional.pad(kp_oct, (0, lcap - kp_oct.shape[1]))
            kp_oct = kp_oct.contiguous()
        q4.update(q_desc=local["desc_lines"], q_has_obs=local.get("has_obs_lines"), q_counts=local.get("counts_lines"), t_kp_octave=kp_oct)
        m4, n4 = self._buf("m4", (B, lcap), i32), self._buf("n4", (B,), i32)
        self.mt_local_line.match_device(plp.MODE_LANDMARKS_LINE, lcap, LL, {**tl, **q4, "t_occupied": t_occupied_lines}, m4, n4, margin=self.margin_local_line,
                                        scale_factors=self.sf_lsd, B=B, stream=st)
        out.update(m4=m4, n4=n4, q4=q4, t_occupied_lines=t_occupied_lines)
        return out

    def _occupied(self, match, counts, has_obs):
        """landmarks_[idx] && landmarks_[idx]->has_observation() after a last-frame call: key point idx < counts[b] holds the landmark of query
        match[idx].  The matcher writes out_match only below the frame's count: the slots past it (whatever the buffer held) are masked before
        anything is gathered with them."""
        torch = self.torch
        hit = match >= 0
        if counts is not None:
            hit &= torch.arange(match.shape[1], device=match.device)[None, :] < counts.to(torch.int64)[:, None]
        if has_obs is None:
            return hit.to(torch.uint8)
        hit &= match < has_obs.shape[1]
        if has_obs.shape[1] == 0:
            return hit.to(torch.uint8)   # all 0: no query, nothing to gather
        q = torch.where(hit, match, torch.zeros_like(match)).long()
        return (hit & (torch.gather(has_obs, 1, q) != 0)).to(torch.uint8)
