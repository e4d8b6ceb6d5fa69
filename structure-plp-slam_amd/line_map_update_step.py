"""The line map update every optimiser of the reference ends with, on one stream, without the host: what the call sites
graph_optimizer.cc:405-417, loop_bundle_adjuster.cc:200-212 / :244-256, global_bundle_adjuster.cc:338-350 and
local_bundle_adjuster_extended_line.cc:652-664 do with a new Pluecker estimate of a line landmark:

  1  torch, on the stream                   pluecker <- the estimate where `moved` (set_PlueckerCoord_without_update_endpoints)
  2  plp_median_depth_device                TRIM_MAX_CHANGE only, where the caller passes no median_depth: compute_median_depth(true) per key frame
  3  plp_trim_line_endpoints_device         endpoint_trimming against the reference key frame's CURRENT pose
  4  torch, on the stream                   pos_w <- the trimmed end points where the status is TRIM_OK (set_pos_in_world_without_update_pluecker);
                                            skip |= out_erase | erase (prepare_for_erasing: the step only raises the flag)
  5  plp_landmark_line_geometry_device      Line::update_information at the new poses and end points

Steps 1 and 4 are torch selections of static shape (torch.where; no .item(), no copy to the host, no boolean-mask indexing).  mode is
TRIM_MAX_CHANGE after the local adjuster and TRIM_DEPTH_POSITIVE after the others; loop_correction_step and loop_ba_step call `run` with the estimate
their transform kernel wrote.  What stays on the host: the line adjusters themselves (the line vertices of the three bundle adjusters), and the map
mutation prepare_for_erasing stands for.

Tables are torch tensors on the step's device, named as landmark_refresh_step names them:
  key frames  pose [F, 15] f64, kl [F, lcap, 68] u8 (_keylsd as plp_keyline), kl_counts [F] or absent, kf_erased [F] u8 or absent; for step 2 kf_lm
              [F, cap] i32 (the landmark row of every key-point slot, -1 = none) and counts [F] or absent
  lines       pluecker_lines [LL, 6] f64 and pos_w_lines [LL, 6] f64 (both updated in place), ref_kf_lines [LL] i32, skip_lines [LL] u8 (updated in
              place; absent: created zero-filled and returned), obs_offsets_lines [LL + 1], obs_kf_lines / obs_idx_lines [T] i32, and the tables
              min_dist_lines / max_dist_lines [LL] f32 (updated in place; a missing one is created zero-filled)
"""
import numpy as np


class line_map_update_step:
    def __init__(self, plp, camera, scale_factor=1.2, num_levels=8, scale_factor_lsd=2.0, num_levels_lsd=1, device_index=0, mt=None):
        import torch
        self.torch, self.plp, self.camera = torch, plp, camera
        self.dev = torch.device("cuda", device_index)

        def table(sf0, n):   # orb_params::calc_scale_factors: float products
            sf = np.ones(n, np.float32)
            for i in range(1, n):
                sf[i] = np.float32(sf[i - 1] * np.float32(sf0))
            return sf
        self.sf, self.sf_lsd = table(scale_factor, num_levels), table(scale_factor_lsd, num_levels_lsd)
        self.mt = mt or plp.matcher(device=device_index)
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def median_depth(self, keyframes, pos_w, stream=None):
        """compute_median_depth(true) of every key frame from kf_lm and the point landmarks' pos_w [L, 3]: [F] f32, the step's buffer"""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        pose, kf_lm = keyframes["pose"], keyframes["kf_lm"]
        F, cap = kf_lm.shape
        med, cnt = self._buf("median", (F,), torch.float32), self._buf("median_count", (F,), torch.int32)
        with torch.cuda.stream(st):
            valid = ((kf_lm >= 0) & (kf_lm < pos_w.shape[0])).to(torch.uint8)
            slots = pos_w[kf_lm.clamp(0, max(pos_w.shape[0] - 1, 0)).to(torch.int64)].contiguous() if pos_w.shape[0] else torch.zeros((F, cap, 3), dtype=torch.float64, device=self.dev)
        self.mt.median_depth_device(F, cap, pose, slots, med, cnt, valid=valid, counts=keyframes.get("counts"), abs_flag=True, stream=st)
        self._keep = (valid, slots)
        return med

    def run(self, keyframes, lines, mode=0, pluecker=None, moved=None, erase=None, median_depth=None, points_pos_w=None, max_change=0.1, stream=None):
        """Enqueue the five steps on `stream` (default: the current stream).  pluecker [LL, 6]: the new estimates, None = pluecker_lines already holds them;
        moved [LL] u8 or None = all: the lines the estimate was written for -- the others are not trimmed; erase [LL] u8 or None: lines the caller's optimiser
        erases besides.  TRIM_MAX_CHANGE: median_depth [F] f32, or points_pos_w [L, 3] with keyframes["kf_lm"].  Returns dict(trim_status [LL] u8: TRIM_*,
        trim_erase [LL] u8, geometry_status_lines [LL] u8 -- the step's own buffers, rewritten by the next run -- and pluecker_lines, pos_w_lines, skip_lines,
        min_dist_lines, max_dist_lines: the caller's tables).  Nothing is synchronised."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        f32, u8 = torch.float32, torch.uint8
        pose, kl = keyframes["pose"], keyframes["kl"]
        pk, pos_w, ref_kf = lines["pluecker_lines"], lines["pos_w_lines"], lines["ref_kf_lines"]
        F, cap, L = pose.shape[0], kl.shape[1], pk.shape[0]

        def table(name, dtype):
            t = lines.get(name)
            if t is None:
                with torch.cuda.stream(st):
                    t = torch.zeros((L,), dtype=dtype, device=self.dev)
            return t
        skip, mn, mx = table("skip_lines", u8), table("min_dist_lines", f32), table("max_dist_lines", f32)
        status, er, geo = self._buf("trim_status", (L,), u8), self._buf("trim_erase", (L,), u8), self._buf("geometry_status_lines", (L,), u8)
        new_pos, trim_skip = self._buf("new_pos", (L, 6), torch.float64), self._buf("trim_skip", (L,), u8)
        if mode == plp.TRIM_MAX_CHANGE and median_depth is None:
            median_depth = self.median_depth(keyframes, points_pos_w, stream=st)
        with torch.cuda.stream(st):
            if pluecker is not None:                         # 1
                pk.copy_(pluecker if moved is None else torch.where(moved.bool().unsqueeze(1), pluecker, pk))
            trim_skip.copy_(skip if moved is None else skip | (moved == 0).to(u8))
            new_pos.copy_(pos_w)
        if L:                                                # 3
            self.mt.trim_line_endpoints_device(self.camera, L, F, cap, pk, ref_kf, lines["obs_offsets_lines"], lines["obs_kf_lines"], lines["obs_idx_lines"], pose, kl,
                                               new_pos, status, er, mode=mode, skip=trim_skip, kf_erased=keyframes.get("kf_erased"), counts=keyframes.get("kl_counts"),
                                               pos_w_old=pos_w if mode == plp.TRIM_MAX_CHANGE else None, median_depth=median_depth, max_change=max_change,
                                               pose_stride=pose.shape[1], stream=st)
        with torch.cuda.stream(st):                          # 4
            if L:
                pos_w.copy_(torch.where((status == plp.TRIM_OK).unsqueeze(1), new_pos, pos_w))
                skip.copy_(skip | er if erase is None else skip | er | (erase != 0).to(u8))
        if L:                                                # 5
            self.mt.landmark_line_geometry_device(F, cap, L, pose, kl, pos_w, ref_kf, lines["obs_offsets_lines"], lines["obs_kf_lines"], lines["obs_idx_lines"], mn, mx,
                                                  geo, self.sf, self.sf_lsd, skip=skip, counts=keyframes.get("kl_counts"), stream=st)
        return dict(trim_status=status, trim_erase=er, geometry_status_lines=geo, pluecker_lines=pk, pos_w_lines=pos_w, skip_lines=skip, min_dist_lines=mn,
                    max_dist_lines=mx)
