"""Loop bundle adjustment: the global adjustment of the point map after a loop closure, its correction carried along the spanning tree, the poses and
positions written back and the landmark geometry refreshed, on one stream.

`loop_ba_step.run` does what module::loop_bundle_adjuster::optimize does for the point map (module/loop_bundle_adjuster.cc:68-181; DESIGN.md section 5,
D23), over the tables local_ba_step and loop_correction_step share:

  1  plp_global_ba_device            every key frame and landmark, num_iter Levenberg-Marquardt iterations without the Huber kernel      :81-86
  2  plp_loop_ba_propagate_device    the correction along kf_parent from the origin; every landmark to its new position                  :109-181
  3  torch, on the stream            pose and pos_w <- the rows step 2 wrote, in place (set_cam_pose, set_pos_in_world)
  4  plp_landmark_geometry_device    landmark::update_normal_and_depth: normal, min_dist, max_dist
  5  plp_loop_ba_propagate_lines_device  with `lines`: an optimised line takes pluecker_after, any other moves with its reference key frame       :184-244
  6  line_map_update_step            the end points trimmed against the poses after the correction (depth mode), written back under the status,
                                     the erased lines flagged in skip_lines, Line::update_information                                    :200-212, :244-256

Step 1 is synchronous with respect to the stream (the entry reads the run's record back after every try); steps 2 - 4 are enqueued.  Nothing branches
on the host: the step's `optimized` bytes start every run as zero, so a run that `stop` ended (status GLOBAL_BA_STOPPED) reaches no key frame in step 2
and every table keeps its values.  With `lines` the line cloud follows on the same stream (a stopped run moves and trims no
line either); without it the step enqueues the four steps above and nothing else.  What stays on the host: the pause of the mapper, the mutexes,
loop_BA_identifier_, and the line vertices of the adjustment itself: whoever ran them hands line_optimized and pluecker_after in.

Tables are torch tensors on the step's device:
  key frames  pose [F, 15] f64 (updated in place), kps [F, cap, 28] u8, x_right [F, cap] f32 or absent, counts [F] or absent, kf_erased [F] u8 or absent,
              kf_is_origin [F] u8, kf_parent [F] i32
  landmarks   pos_w [L, 3] f64 (updated in place), ref_kf [L] i32, skip [L] u8 or absent (will_be_erased), obs_offsets [L + 1], obs_kf / obs_idx [T] i32, and
              the tables normal [L, 3] f64, min_dist / max_dist [L] f32 (updated in place; a missing one is created zero-filled)
  lines       the tables of line_map_update_step, and line_optimized [LL] u8 with pluecker_after [LL, 6] f64 or both absent = no line was optimised; the key
              lines kl [F, lcap, 68] u8 and kl_counts are read from `keyframes`
"""
import numpy as np


class loop_ba_step:
    def __init__(self, plp, camera, setup_type, inv_level_sigma_sq, num_iter=10, scale_factor=1.2, device_index=0, mt=None, scale_factor_lsd=2.0, num_levels_lsd=1):
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.camera, self.setup_type, self.num_iter = camera, int(setup_type), int(num_iter)
        self.sigma = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
        sf = np.ones(len(self.sigma), np.float32)            # orb_params::calc_scale_factors: float products
        for i in range(1, len(sf)):
            sf[i] = np.float32(sf[i - 1] * np.float32(scale_factor))
        self.sf = sf
        self.mt = mt or plp.matcher(device=device_index)
        self._bufs = {}
        self._line_args = dict(camera=camera, scale_factor=scale_factor, num_levels=len(self.sigma), scale_factor_lsd=scale_factor_lsd, num_levels_lsd=num_levels_lsd,
                               device_index=device_index)
        self._line_step = None

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def _lines(self, keyframes, lines, ba, pr, st):
        """steps 5 and 6: dict(line_status [LL] u8: LOOP_BA_LM_*, and what line_map_update_step.run returns)"""
        import importlib
        torch, plp = self.torch, self.plp
        if self._line_step is None:
            mod = importlib.import_module(__package__ + ".line_map_update_step")
            self._line_step = mod.line_map_update_step(plp, mt=self.mt, **self._line_args)
        pk = lines["pluecker_lines"]
        LL, F = pk.shape[0], keyframes["pose"].shape[0]
        pk_new, lst = self._buf("pluecker_new", (LL, 6), torch.float64), self._buf("line_status", (LL,), torch.uint8)
        with torch.cuda.stream(st):
            pk_new.copy_(pk)
        if LL:
            self.mt.loop_ba_propagate_lines_device(LL, F, pr["pose"], pr["pose_before"], pr["kf_status"], pk, lines["ref_kf_lines"], pk_new, lst,
                                                   line_optimized=lines.get("line_optimized"), pluecker_after=lines.get("pluecker_after"),
                                                   lm_erased=lines.get("skip_lines"), stream=st)
        with torch.cuda.stream(st):
            ran = ba["status"][0] != plp.GLOBAL_BA_STOPPED
            moved = (((lst == plp.LOOP_BA_LM_OPTIMIZED) | (lst == plp.LOOP_BA_LM_MOVED)) & ran).to(torch.uint8)
        r = self._line_step.run(keyframes, lines, mode=plp.TRIM_DEPTH_POSITIVE, pluecker=pk_new, moved=moved, stream=st)
        return dict(r, line_status=lst)

    def run(self, keyframes, landmarks, stop=None, stream=None, lines=None):
        """Returns dict(status [1] u8: GLOBAL_BA_*, info [4], chi2 [3], kf_optimized [F], lm_optimized [L], kf_status [F] u8: LOOP_BA_KF_*, lm_status [L] u8:
        LOOP_BA_LM_*, pose_before [F, 12], geometry_status [L] u8 -- the step's own buffers, rewritten by the next run -- and pose, pos_w, normal, min_dist,
        max_dist: the caller's tables, which local_map_step reads next; with `lines` also line_status [LL] u8: LOOP_BA_LM_* and the results of
        line_map_update_step.run).  stop: None or a host int32 array of one element."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8
        pose, pos_w = keyframes["pose"], landmarks["pos_w"]
        F, L, cap = pose.shape[0], pos_w.shape[0], keyframes["kps"].shape[1]
        T = landmarks["obs_kf"].shape[0]
        ba = dict(status=self._buf("status", (1,), u8), kf_optimized=self._buf("kf_optimized", (F,), u8), lm_optimized=self._buf("lm_optimized", (L,), u8),
                  pose=self._buf("pose_after", (F, 15), f64), pos_w=self._buf("pos_after", (L, 3), f64), info=self._buf("info", (4,), i32),
                  chi2=self._buf("chi2", (3,), f64))
        with torch.cuda.stream(st):
            for k in ("kf_optimized", "lm_optimized", "info", "chi2"):
                ba[k].zero_()
        # 1: the adjustment (Huber off, :81)
        self.mt.global_ba_device(self.camera, self.setup_type, F, L, T, cap, pose, keyframes["kps"], pos_w, landmarks["obs_offsets"], landmarks["obs_kf"],
                                 landmarks["obs_idx"], self.sigma, {k: v for k, v in ba.items() if v.numel()}, x_right=keyframes.get("x_right"),
                                 counts=keyframes.get("counts"), kf_erased=keyframes.get("kf_erased"), kf_is_origin=keyframes["kf_is_origin"],
                                 lm_erased=landmarks.get("skip"), pose_stride=pose.shape[1], num_iter=self.num_iter, use_huber_kernel=False, stop=stop, stream=st)
        # 2: the map update into buffers that start as the tables (a lane reads its ancestors' poses from the table while others write)
        pr = dict(pose=self._buf("pose_new", (F, 15), f64), pose_before=self._buf("pose_before", (F, 12), f64), kf_status=self._buf("kf_status", (F,), u8),
                  pos_w=self._buf("pos_new", (L, 3), f64), lm_status=self._buf("lm_status", (L,), u8))
        with torch.cuda.stream(st):
            pr["pose"].copy_(pose[:, :15])
            pr["pose_before"].copy_(pose[:, :12])
            pr["pos_w"].copy_(pos_w)
        self.mt.loop_ba_propagate_device(F, L, pose, keyframes["kf_parent"], ba["kf_optimized"], ba["pose"], pos_w, landmarks["ref_kf"], ba["lm_optimized"],
                                         ba["pos_w"], pr, kf_erased=keyframes.get("kf_erased"), kf_is_origin=keyframes["kf_is_origin"],
                                         lm_erased=landmarks.get("skip"), pose_stride=pose.shape[1], stream=st)
        with torch.cuda.stream(st):
            # 3: the write-back; rows step 2 did not write still hold what they held
            pose[:, :15].copy_(pr["pose"])
            pos_w.copy_(pr["pos_w"])

        def table(name, shape, dtype):
            t = landmarks.get(name)
            if t is None:
                with torch.cuda.stream(st):
                    t = torch.zeros(shape, dtype=dtype, device=self.dev)
            return t
        normal, mn, mx = table("normal", (L, 3), f64), table("min_dist", (L,), f32), table("max_dist", (L,), f32)
        geo = self._buf("geometry_status", (L,), u8)
        # 4: update_normal_and_depth at the new poses and positions
        if L:
            self.mt.landmark_geometry_device(F, cap, L, pose, keyframes["kps"], pos_w, landmarks["ref_kf"], landmarks["obs_offsets"], landmarks["obs_kf"],
                                             landmarks["obs_idx"], normal, mn, mx, geo, self.sf, skip=landmarks.get("skip"), counts=keyframes.get("counts"), stream=st)
        res = dict(status=ba["status"], info=ba["info"], chi2=ba["chi2"], kf_optimized=ba["kf_optimized"], lm_optimized=ba["lm_optimized"],
                   kf_status=pr["kf_status"], lm_status=pr["lm_status"], pose_before=pr["pose_before"], geometry_status=geo, pose=pose, pos_w=pos_w, normal=normal,
                   min_dist=mn, max_dist=mx)
        if lines is not None:
            res.update(self._lines(keyframes, lines, ba, pr, st))
        return res
