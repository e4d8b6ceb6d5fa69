"""Loop correction: the pose graph of a detected loop optimised, the key-frame poses written back and the landmarks moved with their reference key
frames, on one stream, without the host.

`loop_correction_step.run` does what global_optimization_module::correct_loop does from optimize::graph_optimizer::optimize on
(optimize/graph_optimizer.cc:53-350):

  1  plp_pose_graph_optimize_device   vertices, edges, 50 Levenberg-Marquardt iterations: Sim3_cw, corrected_Sim3_wc and the pose rows     :58-328
  2  torch, on the stream             pose <- the pose row where the problem was solved and the row is a vertex (set_cam_pose, :325)
  3  plp_correct_landmarks_device     pos_w <- corrected_Sim3_wc[ref].map(Sim3_cw[ref].map(pos_w)), in place                              :331-348
  4  plp_landmark_geometry_device     landmark::update_normal_and_depth: normal, min_dist, max_dist                                      :349
  5  plp_correct_landmark_lines_device  with `lines`: pluecker <- (corrected_Sim3_wc_pluecker * Sim3_cw_pluecker) * pluecker                :352-403
  6  line_map_update_step             the end points trimmed against the corrected poses (depth mode), written back under the status, the erased
                                      lines flagged in skip_lines, Line::update_information                                              :405-417

Step 2 is a torch selection of static shape (no .item(), no copy to the host, no boolean-mask indexing).  A problem the optimiser does not solve
(a cap that is too small, a loop key frame that is no vertex: `status`) changes nothing: the step's Sim3 buffers start every run as the identity,
which maps a landmark onto itself exactly, and the pose rows are kept.  The descriptors do not change with the geometry; landmark_refresh_step
computes them.  With `lines` the line cloud of :352-419 follows on the same stream (a problem that is not solved moves and
trims no line either); without it the step enqueues the four steps above and nothing else.  What stays on the host: add_loop_edge, the global bundle
adjustment that follows.

Tables are torch tensors on the step's device, named as landmark_refresh_step and covisibility_step name them:
  key frames  pose [F, 15] f64 (updated in place), kps [F, cap, 28] u8, counts [F] or absent, kf_erased [F] u8, kf_id [F] i32, kf_parent [F] i32,
              kf_conn / kf_conn_w [F, conn_cap] i32, kf_n_conn [F], kf_covis_all (or kf_covis) / kf_covis_w [F, covis_cap] i32, kf_n_covis [F],
              kf_loop_offsets [F + 1] i32 and kf_loop, or absent = no loop edges
  landmarks   pos_w [L, 3] f64 (updated in place), ref_kf [L] i32, corr_kf [L] i32 or absent = ref_kf (the row of ref_keyfrm_id_in_loop_fusion_ where the
              landmark was fused by this loop), skip [L] u8 or absent, obs_offsets [L + 1], obs_kf / obs_idx [T] i32, and the tables normal [L, 3] f64,
              min_dist / max_dist [L] f32 (updated in place; a missing one is created zero-filled)
  lines       the tables of line_map_update_step, and corr_kf_lines [LL] i32 or absent = ref_kf_lines; the key lines kl [F, lcap, 68] u8 and kl_counts are
              read from `keyframes`
  problem     the arrays of plp.pose_graph_problems for one problem, on the device
"""
import numpy as np


class loop_correction_step:
    def __init__(self, plp, edge_cap=4096, env_cap=16384, scale_factor=1.2, num_levels=8, max_iter=50, device_index=0, mt=None, camera=None, scale_factor_lsd=2.0,
                 num_levels_lsd=1):
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.edge_cap, self.env_cap, self.max_iter = int(edge_cap), int(env_cap), int(max_iter)
        sf = np.ones(num_levels, np.float32)                 # orb_params::calc_scale_factors: float products
        for i in range(1, num_levels):
            sf[i] = np.float32(sf[i - 1] * np.float32(scale_factor))
        self.sf = sf
        self.mt = mt or plp.matcher(device=device_index)
        self._bufs = {}
        self._line_args = dict(camera=camera, scale_factor=scale_factor, num_levels=num_levels, scale_factor_lsd=scale_factor_lsd, num_levels_lsd=num_levels_lsd,
                               device_index=device_index)
        self._line_step = None

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def _lines(self, keyframes, lines, o, st):
        """steps 5 and 6: dict(line_status [LL] u8: CORRECT_LINE_*, and what line_map_update_step.run returns)"""
        import importlib
        torch, plp = self.torch, self.plp
        if self._line_args["camera"] is None:
            raise plp.PlpError(plp.PLP_ERR_INVALID_ARG, "loop_correction_step needs camera= to move line landmarks")
        if self._line_step is None:
            mod = importlib.import_module(__package__ + ".line_map_update_step")
            self._line_step = mod.line_map_update_step(plp, mt=self.mt, **self._line_args)
        pk = lines["pluecker_lines"]
        LL, F = pk.shape[0], keyframes["pose"].shape[0]
        pk_new, lst = self._buf("pluecker_new", (LL, 6), torch.float64), self._buf("line_status", (LL,), torch.uint8)
        with torch.cuda.stream(st):
            pk_new.copy_(pk)
        if LL:
            self.mt.correct_landmark_lines_device(LL, F, pk, lines["ref_kf_lines"], o["sim3_cw"], o["corrected_wc"], pk_new, lst, corr_kf=lines.get("corr_kf_lines"),
                                                  lm_erased=lines.get("skip_lines"), kf_erased=keyframes.get("kf_erased"), stream=st)
        with torch.cuda.stream(st):
            solved = o["status"][0] == plp.POSE_GRAPH_OK
            moved = ((lst == plp.CORRECT_LINE_OK) & solved).to(torch.uint8)
            erase = ((lst == plp.CORRECT_LINE_NO_REF) & solved).to(torch.uint8)
        r = self._line_step.run(keyframes, lines, mode=plp.TRIM_DEPTH_POSITIVE, pluecker=pk_new, moved=moved, erase=erase, stream=st)
        return dict(r, line_status=lst)

    def run(self, keyframes, landmarks, problem, stream=None, lines=None):
        """Enqueue the four steps on `stream` (default: the current stream).  Returns dict(status [1] u8: POSE_GRAPH_*, num_edges [1], info [1, 4], chi2 [1, 2],
        sim3_cw, corrected_wc [F, 8], lm_status [L] u8: CORRECT_LM_*, geometry_status [L] u8 -- the step's own buffers, rewritten by the next run -- and pose,
        pos_w, normal, min_dist, max_dist: the caller's tables; with `lines` also line_status [LL] u8: CORRECT_LINE_* and the results of
        line_map_update_step.run).  Nothing is synchronised."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        f64, f32, i32, u8 = torch.float64, torch.float32, torch.int32, torch.uint8
        pose, pos_w = keyframes["pose"], landmarks["pos_w"]
        F, L, cap = pose.shape[0], pos_w.shape[0], keyframes["kps"].shape[1]
        covis = keyframes["kf_covis_all"] if keyframes.get("kf_covis_all") is not None else keyframes["kf_covis"]
        o = dict(status=self._buf("status", (1,), u8), num_edges=self._buf("num_edges", (1,), i32), sim3_cw=self._buf("sim3_cw", (1, F, 8), f64),
                 corrected_wc=self._buf("corrected_wc", (1, F, 8), f64), pose=self._buf("pose", (1, F, 15), f64), info=self._buf("info", (1, 4), i32),
                 chi2=self._buf("chi2", (1, 2), f64))
        ident = self._buf("ident", (8,), f64)
        with torch.cuda.stream(st):
            ident.zero_()
            ident[3:8:4] = 1.0                               # quaternion w and the scale
            o["sim3_cw"].copy_(ident.expand(1, F, 8))
            o["corrected_wc"].copy_(ident.expand(1, F, 8))
            o["pose"].copy_(pose[:, :15].unsqueeze(0))
            o["info"].zero_()
            o["chi2"].zero_()
            o["num_edges"].zero_()
        tables = dict(keyframes, kf_covis=covis)
        # 1: the optimisation
        self.mt.pose_graph_optimize_device(1, F, tables, problem, o, keyframes["kf_conn"].shape[1], covis.shape[1], self.edge_cap, self.env_cap,
                                           pose_stride=pose.shape[1], max_iter=self.max_iter, stream=st)
        with torch.cuda.stream(st):
            # 2: set_cam_pose for every vertex of a solved problem; the rows the optimiser did not write still hold the pose they had
            pose[:, :15].copy_(o["pose"][0])
        # 3: the landmarks follow their key frames
        lm_status = self._buf("lm_status", (L,), u8)
        corr = landmarks.get("corr_kf")
        if L:
            self.mt.correct_landmarks_device(L, F, pos_w, corr if corr is not None else landmarks["ref_kf"], o["sim3_cw"], o["corrected_wc"], pos_w, lm_status,
                                             lm_erased=landmarks.get("skip"), kf_erased=keyframes.get("kf_erased"), stream=st)

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
        res = dict(status=o["status"], num_edges=o["num_edges"], info=o["info"], chi2=o["chi2"], sim3_cw=o["sim3_cw"][0], corrected_wc=o["corrected_wc"][0],
                   lm_status=lm_status, geometry_status=geo, pose=pose, pos_w=pos_w, normal=normal, min_dist=mn, max_dist=mx)
        if lines is not None:
            res.update(self._lines(keyframes, lines, o, st))
        return res
