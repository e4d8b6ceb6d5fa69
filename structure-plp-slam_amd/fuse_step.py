"""The mapping thread's landmark fusion search for G target key frames at once: landmark tables and poses in, best key point / key line per
landmark and target out, on one stream, without the host.

For G target key frames whose features are already in HBM, `fuse_step.run` does what mapping_module::fuse_landmark_duplication and
fuse_landmark_duplication_line (mapping_module.cc:704-805) do per target with match::fuse::replace_duplication[_line] (match/fuse.cc:169-298,
335-470), up to the point where the reference starts to change the map:

  1  plp_project_landmarks_device        -> PLP_MATCH_MODE_FUSE        replace_duplication       the current key frame's point landmarks
  2  plp_project_landmark_lines_device   -> PLP_MATCH_MODE_FUSE_LINE   replace_duplication_line  the current key frame's line landmarks

The landmark tables are shared by the G targets (plp_project_args.shared_landmarks): this is the forward pass, the current key frame's landmarks
into every target.  The reverse pass -- the union of the targets' landmarks into the current key frame -- is the same call with G = 1; its list
is long (targets x key points, about 40 000).  No launch dimension limits the number of landmarks per problem: the projection runs m / 256
workgroups along x (points) or walks the list in chunks inside one workgroup (lines), the search m / 4 workgroups along x, and
plp_match_args limits only the targets' n_cap (8 192); so the step does not split a list.  G is at most 65 535 (the y dimension of both grids).

The projections write q_valid / q_reproj_d / q_x_right / q_level in the layout the search reads, so nothing is copied or compacted between
the two calls.  The search reads one descriptor row per (target, landmark): the shared descriptors are expanded to G x m on the stream (a device
copy into a buffer the step keeps).

What stays on the host: the skip flags (`!lm`, will_be_erased(), is_observed_in_keyframe: they read landmark objects) and everything after the
search -- fuse.cc:300-325 / 472-497, which replaces the landmark with fewer observations or adds the observation (landmark::replace,
add_observation, keyframe::add_landmark); it mutates the map in list order and is not part of the step.

Tables are torch tensors on the step's device:
  targets    kps [G, cap, 28] u8 (undist_keypts_ as plp_keypoint), desc [G, cap, 32], counts [G], x_right [G, cap] f32 or None (stereo_x_right_),
             kl [G, lcap, 68] u8 (_keylsd as plp_keyline), lbd [G, lcap, 32], kl_counts [G]
  landmarks  points: pos_w [m, 3] f64, normal [m, 3] f64, min_dist / max_dist [m] f32, desc [m, 32] u8, skip [G, m] u8 or None;
             lines: pos_w_lines [ml, 6] f64, min_dist_lines / max_dist_lines [ml] f32, desc_lines [ml, 32] u8, skip_lines [G, ml] u8 or None
  pose       [G, 15] f64: frame_pose rows of the targets (rot_cw, trans_cw, cam_center)
"""
import math

import numpy as np


class fuse_step:
    def __init__(self, plp, camera, scale_factor=1.2, num_levels=8, scale_factor_lsd=2.0, num_levels_lsd=1, margin=3.0, margin_line=10.0,
                 device_index=0):
        """camera: a plp.camera_model.  The margins default to what mapping_module.cc:704-805 passes: 3.0 for points (replace_duplication's own
        default) and 10.0 for lines."""
        import torch
        self.torch, self.plp, self.camera = torch, plp, camera
        self.dev = torch.device("cuda", device_index)
        self.margin, self.margin_line = float(margin), float(margin_line)
        f32 = np.float32

        def tables(sf0, n):   # orb_params::calc_scale_factors / calc_inv_level_sigma_sq: float products, 1.0f / (sf * sf)
            sf = np.ones(n, np.float32)
            for i in range(1, n):
                sf[i] = f32(sf[i - 1] * f32(sf0))
            inv = np.array([f32(1.0) / f32(s * s) for s in sf], np.float32)
            return sf, inv
        self.sf, self.inv_sigma = tables(scale_factor, num_levels)
        self.sf_lsd, self.inv_sigma_lsd = tables(scale_factor_lsd, num_levels_lsd)
        self.log_sf = f32(math.log(f32(scale_factor)))                 # keyframe::log_scale_factor_ (logf as D5 defines it)
        self.log_sf_lsd = f32(math.log(f32(scale_factor_lsd)))
        self.num_levels, self.num_levels_lsd = int(num_levels), int(num_levels_lsd)
        self.grid = camera.grid()
        self.mt = plp.matcher(device=device_index)
        self.mt_line = plp.matcher(device=device_index)
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def run(self, targets, landmarks, pose, stream=None, points=True, lines=True):
        """Enqueue both chains for the G targets on `stream` (default: the current stream).  Returns dict(best [G, m] i32, best_lines [G, ml] i32:
        out_query_best of the two searches -- the target's key point / key line a landmark would fuse with, -1 = none or not a valid query --
        and the query arrays under q / q_lines (q_valid, q_status, ...)).  Nothing is synchronised; the returned tensors are the step's own
        buffers, rewritten by the next run."""
        torch, plp, cam = self.torch, self.plp, self.camera
        st = stream or torch.cuda.current_stream(self.dev)
        G = pose.shape[0]
        i32, f32, f64, u8 = torch.int32, torch.float32, torch.float64, torch.uint8
        out = {}
        if points:
            m, cap = landmarks["pos_w"].shape[0], targets["kps"].shape[1]
            q = dict(q_reproj_d=self._buf("q_reproj_d", (G, m, 2), f64), q_x_right=self._buf("q_xr", (G, m), f32), q_level=self._buf("q_level", (G, m), i32),
                     q_valid=self._buf("q_valid", (G, m), u8))
            status = self._buf("q_status", (G, m), u8)
            best = self._buf("best", (G, m), i32)
            if m > 0:
                self.mt.project_landmarks_device(cam, G, m, pose, landmarks["pos_w"], landmarks["min_dist"], landmarks["max_dist"], q["q_valid"],
                                                 out_reproj_d=q["q_reproj_d"], obs_mean_normal=landmarks["normal"], skip=landmarks.get("skip"),
                                                 out_x_right=q["q_x_right"], out_level=q["q_level"], out_status=status, shared_landmarks=True,
                                                 dist_mode=plp.PROJECT_DIST_CENTER, ray_test=True, log_scale_factor=self.log_sf, num_levels=self.num_levels,
                                                 stream=st)
                with torch.cuda.stream(st):   # one descriptor row per (target, landmark), as the search reads them
                    qd = self._buf("q_desc", (G, m, 32), u8)
                    qd.copy_(landmarks["desc"].unsqueeze(0).expand(G, m, 32))
                fields = dict(t_kps=targets["kps"], t_desc=targets["desc"], t_counts=targets.get("counts"), t_x_right=targets.get("x_right"), q_desc=qd,
                              inv_level_sigma_sq=self.inv_sigma, **q)
                self._fuse(self.mt, plp.MODE_FUSE, G, cap, m, fields, best, self.margin, self.sf, self.grid, st)
            out.update(best=best, q={**q, "q_status": status})
        if lines:
            ml, lcap = landmarks["pos_w_lines"].shape[0], targets["kl"].shape[1]
            q = dict(q_reproj_d=self._buf("ql_sp_d", (G, ml, 2), f64), q_reproj2_d=self._buf("ql_ep_d", (G, ml, 2), f64),
                     q_level=self._buf("ql_level", (G, ml), i32), q_valid=self._buf("ql_valid", (G, ml), u8))
            status = self._buf("ql_status", (G, ml), u8)
            best = self._buf("best_lines", (G, ml), i32)
            if ml > 0:
                self.mt_line.project_landmark_lines_device(cam, G, ml, pose, landmarks["pos_w_lines"], landmarks["min_dist_lines"], landmarks["max_dist_lines"],
                                                           q["q_valid"], out_reproj_sp_d=q["q_reproj_d"], out_reproj_ep_d=q["q_reproj2_d"],
                                                           skip=landmarks.get("skip_lines"), out_level=q["q_level"], out_status=status, shared_landmarks=True,
                                                           line_dist_mode=plp.PROJECT_LINE_ENDPOINTS, log_scale_factor=self.log_sf_lsd,
                                                           num_levels=self.num_levels_lsd, stream=st)
                with torch.cuda.stream(st):
                    qd = self._buf("ql_desc", (G, ml, 32), u8)
                    qd.copy_(landmarks["desc_lines"].unsqueeze(0).expand(G, ml, 32))
                fields = dict(t_kl=targets["kl"], t_desc=targets["lbd"], t_counts=targets.get("kl_counts"), q_desc=qd, inv_level_sigma_sq=self.inv_sigma_lsd, **q)
                self._fuse(self.mt_line, plp.MODE_FUSE_LINE, G, lcap, ml, fields, best, self.margin_line, self.sf_lsd, None, st)
            out.update(best_lines=best, q_lines={**q, "q_status": status})
        return out

    def _fuse(self, mt, mode, G, n_cap, m, fields, best, margin, sf, grid, st):
        """plp_match_device in a fuse mode: out_query_best instead of out_match / out_num.  A target set without slots (n_cap 0) matches nothing."""
        if n_cap == 0:
            with self.torch.cuda.stream(st):
                best.fill_(-1)
            return
        fields = {k: v for k, v in fields.items() if v is not None}
        fields["out_query_best"] = best
        mt.match_device(mode, n_cap, m, fields, best, best, margin=margin, scale_factors=sf, grid=grid, B=G, stream=st)
