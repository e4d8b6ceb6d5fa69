"""Refresh of the landmark tables after the map's geometry has changed: key-frame tables, poses, positions and observation lists in, descriptors,
mean viewing directions and valid distance ranges out, on one stream, without the host.

For L point landmarks and LL line landmarks over a table of F key frames whose features are already in HBM, `landmark_refresh_step.run` does what
the loops of mapping_module::update_new_keyframe (mapping_module.cc:619-650) do per landmark -- and what follows every bundle adjustment
(optimize/local_bundle_adjuster_extended_line.cc:632-660) and a map load:

  1  gather       the descriptor rows of a landmark's observations whose key frame will not be erased, packed with offsets of their own
                  (landmark.cc:201-210: compute_descriptor leaves erased key frames out; update_normal_and_depth does not)
  2  plp_landmark_descriptor_device         landmark::compute_descriptor / Line::compute_descriptor, the search
  3  copy         the chosen row into desc [L, 32] where there is one and the landmark is not skipped
  4  plp_landmark_geometry_device           landmark::update_normal_and_depth        normal, min_dist, max_dist, status
     plp_landmark_line_geometry_device      Line::update_information                 min_dist_lines, max_dist_lines, status_lines

Steps 1 and 3 are torch index operations of static shape on the step's stream (no .item(), no copy to the host, no boolean-mask indexing): the
packed rows live in a buffer of as many rows as there are observations plus one, where the rows that are left out go.  The outputs are the landmark
tables fuse_step and posed_step read (normal, min_dist, max_dist, desc; *_lines), so that after create_landmarks_step or an optimiser's result
uploaded once the chain  positions -> tables -> observe / project -> match  never leaves HBM.  Rows the reference leaves alone (a skipped landmark,
one without observations, one whose status is not LG_UPDATED) keep their values.

plp_landmark_descriptor_* takes at most 1024 rows per landmark; a landmark has at most one observation per key frame, so the step raises for
F > 1024 instead of checking lists on the device.

What stays on the host: the map mutation around these calls (add_observation, replace, prepare_for_erasing, the choice of a new ref_keyfrm_ in
erase_observation) -- the caller flattens the observations_ maps in their iteration order.

Tables are torch tensors on the step's device:
  key frames  kps [F, cap, 28] u8 (undist_keypts_ as plp_keypoint), desc [F, cap, 32], counts [F], pose [F, 15] f64 (frame_pose rows),
              kl [F, lcap, 68] u8 (_keylsd as plp_keyline), lbd [F, lcap, 32], kl_counts [F]; kf_erased [F] u8 (keyframe::will_be_erased())
  landmarks   points: pos_w [L, 3] f64, ref_kf [L] i32, skip [L] u8 or None, obs_offsets [L + 1] i32, obs_kf / obs_idx [T] i32, and the tables
              desc [L, 32] u8, normal [L, 3] f64, min_dist / max_dist [L] f32 (updated in place; a missing one is created zero-filled);
              lines: pos_w_lines [LL, 6], ref_kf_lines, skip_lines, obs_offsets_lines, obs_kf_lines, obs_idx_lines, desc_lines, min_dist_lines,
              max_dist_lines
"""
import numpy as np


class landmark_refresh_step:
    def __init__(self, plp, scale_factor=1.2, num_levels=8, scale_factor_lsd=2.0, num_levels_lsd=1, device_index=0):
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)

        def table(sf0, n):   # orb_params::calc_scale_factors: float products
            sf = np.ones(n, np.float32)
            for i in range(1, n):
                sf[i] = np.float32(sf[i - 1] * np.float32(sf0))
            return sf
        self.sf, self.sf_lsd = table(scale_factor, num_levels), table(scale_factor_lsd, num_levels_lsd)
        self.mt = plp.matcher(device=device_index)
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def run(self, keyframes, landmarks, stream=None, points=True, lines=True):
        """Enqueue the refresh of both landmark lists on `stream` (default: the current stream).  Returns dict(desc, normal, min_dist, max_dist,
        status [L] u8, best_idx [L] i32 and the same with _lines, without a normal): the landmark tables, which are the caller's tensors where
        `landmarks` holds them, and the step's own buffers (status, best_idx), rewritten by the next run.  Nothing is synchronised."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        F = keyframes["pose"].shape[0]
        if F > 1024:
            raise self.plp.PlpError(self.plp.PLP_ERR_UNSUPPORTED, "more than 1024 key frames: plp_landmark_descriptor_* takes at most 1024 rows per landmark")
        out = {}
        if points:
            out.update(self._refresh(st, False, "", F, keyframes["kps"], keyframes["desc"], keyframes.get("counts"), keyframes, landmarks))
        if lines:
            out.update(self._refresh(st, True, "_lines", F, keyframes["kl"], keyframes["lbd"], keyframes.get("kl_counts"), keyframes, landmarks))
        return out

    def _refresh(self, st, lines, sfx, F, feats, fdesc, counts, keyframes, landmarks):
        torch = self.torch
        i32, i64, f32, f64, u8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.uint8
        pos_w, ref_kf, skip = landmarks["pos_w" + sfx], landmarks["ref_kf" + sfx], landmarks.get("skip" + sfx)
        off, obs_kf, obs_idx = landmarks["obs_offsets" + sfx], landmarks["obs_kf" + sfx], landmarks["obs_idx" + sfx]
        L, T, cap = pos_w.shape[0], obs_kf.shape[0], feats.shape[1]

        def table(name, shape, dtype):
            t = landmarks.get(name + sfx)
            if t is None:
                with torch.cuda.stream(st):
                    t = torch.zeros(shape, dtype=dtype, device=self.dev)
            return t
        desc = table("desc", (L, 32), u8)
        mn, mx = table("min_dist", (L,), f32), table("max_dist", (L,), f32)
        normal = None if lines else table("normal", (L, 3), f64)
        status, best = self._buf("status" + sfx, (L,), u8), self._buf("best" + sfx, (L,), i32)
        res = {"desc" + sfx: desc, "min_dist" + sfx: mn, "max_dist" + sfx: mx, "status" + sfx: status, "best_idx" + sfx: best}
        if not lines:
            res["normal"] = normal
        if L == 0:
            return res
        packed, off2 = self._buf("packed" + sfx, (T + 1, 32), u8), self._buf("off2" + sfx, (L + 1,), i32)
        with torch.cuda.stream(st):
            # 1: the rows of the key frames that stay, in list order, packed; row T takes the ones that are left out
            kf, ix = obs_kf.to(i64), obs_idx.to(i64)
            inside = (kf >= 0) & (kf < F) & (ix >= 0) & (ix < cap)          # an index outside the table is not followed (the geometry entry reports it)
            kfc, ixc = kf.clamp(0, F - 1), ix.clamp(0, max(cap - 1, 0))
            keep = inside & (keyframes["kf_erased"].to(i64)[kfc] == 0)
            before = torch.zeros(T + 1, dtype=i64, device=self.dev)
            before[1:] = torch.cumsum(keep.to(i64), 0)                      # kept rows in front of observation o
            off2.copy_(before[off.to(i64)])
            if T and cap:
                rows = fdesc.reshape(F * cap, 32)[kfc * cap + ixc]
                packed.index_copy_(0, torch.where(keep, before[:T], torch.full_like(kf, T)), rows)
        # 2: the search
        self.mt.landmark_descriptors_device(packed, off2, L, best, stream=st)
        with torch.cuda.stream(st):
            # 3: descriptor_ = descriptors.at(best_idx).clone() -- where compute_descriptor got that far
            take = best >= 0
            if skip is not None:
                take = take & (skip == 0)
            src = packed[(off2[:L].to(i64) + best.to(i64)).clamp(0, T)]
            desc.copy_(torch.where(take.unsqueeze(1), src, desc))
        # 4: normals and distance ranges
        if lines:
            self.mt.landmark_line_geometry_device(F, cap, L, keyframes["pose"], feats, pos_w, ref_kf, off, obs_kf, obs_idx, mn, mx, status, self.sf,
                                                  self.sf_lsd, skip=skip, counts=counts, stream=st)
        else:
            self.mt.landmark_geometry_device(F, cap, L, keyframes["pose"], feats, pos_w, ref_kf, off, obs_kf, obs_idx, normal, mn, mx, status, self.sf,
                                             skip=skip, counts=counts, stream=st)
        return res
