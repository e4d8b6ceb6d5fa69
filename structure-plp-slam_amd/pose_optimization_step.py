"""The tracker's frame from the last-frame match to the tracked-landmark count, on one stream, without the host.

For B frames `tracked_pose_step.run` does what module/frame_tracker.cc:56-106 (motion_based_track) and tracking_module.cc:700-816
(optimize_current_frame_with_local_map) do per frame, between the poses and landmark tables going in and the optimised pose coming out:

  1  posed_tracker_step.run_last_frame    calls 1 and 2 of posed_step.py: the last frame's landmarks projected and matched (points, lines)
  2  torch, on the stream                 the slot form of the optimiser: for every key point / key line the landmark row it got, `valid`, pos_w
  3  plp_pose_optimize_device             pose_optimizer[_extended_line]::optimize from the predicted pose                  frame_tracker.cc:83-96
  4  torch                                the array half of discard_outliers[_line]: a flagged slot loses its landmark       :259-314
  5  posed_tracker_step.run_local         calls 3 and 4 with the optimised pose and the surviving occupancy
  6  torch, plp_pose_optimize_device      the slot form again (a local match replaces what the slot held), the optimiser    tracking_module.cc:750-759
  7  torch                                num_tracked_lms_ / _num_tracked_lms_line: slots with a landmark that is no outlier  :761-816

Static shapes, no .item(), no boolean-mask indexing: nothing is synchronised and nothing returns to the host.  The host's writes to landmark
objects (is_observable_in_tracking_, increase_num_observed, the widened second search) are not part of the step.  The tables are
posed_step.py's, and `last` / `local` carry `plucker_lines` [B, m, 6] f64 beside `pos_w_lines` (landmark_line::get_PlueckerCoord(): the line edge reads
Pluecker coordinates, the matchers end points); they may carry `erased` / `erased_lines` [B, m] u8 (will_be_erased() of the row), which the optimiser's `valid`
honours.
"""
import importlib

import numpy as np


class tracked_pose_step:
    def __init__(self, plp, camera, setup_type, num_trials=4, num_each_iter=10, use_lines=True, **posed_kw):
        """camera, setup_type and posed_kw: as posed_tracker_step.  use_lines: map_db_->_b_use_line_tracking (False: pose_optimizer, the line
        matches still run)."""
        posed = importlib.import_module(__package__ + ".posed_step")
        self.plp, self.camera, self.setup_type = plp, camera, int(setup_type)
        self.posed = posed.posed_tracker_step(plp, camera, setup_type, **posed_kw)
        self.torch, self.dev = self.posed.torch, self.posed.dev
        self.num_trials, self.num_each_iter, self.use_lines = int(num_trials), int(num_each_iter), bool(use_lines)
        f32 = np.float32
        # orb_params::calc_inv_level_sigma_sq: 1.0f / (scale_factor * scale_factor), floats
        self.inv_sigma_sq = np.array([f32(1.0) / f32(s * s) for s in self.posed.sf], np.float32)
        self.inv_sigma_sq_lsd = np.array([f32(1.0) / f32(s * s) for s in self.posed.sf_lsd], np.float32)
        self.mt = plp.matcher(device=self.dev.index or 0)
        self._bufs = {}

    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[name] = t
        return t

    def _hit(self, match, counts, rows):
        torch = self.torch
        return (match >= 0) & (match < rows) & (torch.arange(match.shape[1], device=match.device)[None, :] < counts.to(torch.int64)[:, None])

    def gather(self, match, counts, table, pos_key, erased_key):
        """(valid [B, cap] bool, pos_w [B, cap, D] f64, row [B, cap] i64): what the key point / key line of every slot got from `table`"""
        torch = self.torch
        pos = table[pos_key]
        hit = self._hit(match, counts, pos.shape[1])
        if pos.shape[1] == 0:
            return hit & False, torch.zeros(match.shape + (pos.shape[2],), dtype=pos.dtype, device=pos.device), match.long() * 0
        q = torch.where(hit, match, torch.zeros_like(match)).long()
        er = table.get(erased_key)
        valid = hit if er is None else hit & (torch.gather(er, 1, q) == 0)
        return valid, torch.gather(pos, 1, q[..., None].expand(-1, -1, pos.shape[2])), q

    def _optimize(self, tag, frame, pose_in, valid, pos_w, valid_l, pos_w_l, st):
        torch, plp = self.torch, self.plp
        B, cap = valid.shape
        lcap = valid_l.shape[1] if self.use_lines else 0
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
        o = {k: self._buf(f"{tag}_{k}", (B,) + shape(cap, lcap, self.num_trials), tt[dt]) for k, (shape, dt, _) in plp.POSE_OPT_OUTPUTS.items()}
        with torch.cuda.stream(st):
            o["outlier"].zero_(); o["outlier_lines"].zero_()          # a slot without an observation has no flag
            v, pw = valid.to(torch.uint8).contiguous(), pos_w.contiguous()
            vl, pwl = valid_l.to(torch.uint8).contiguous(), pos_w_l.contiguous()
        kw = {}
        if lcap:
            kw = dict(l_cap=lcap, line_valid=vl, keylines=frame["kl"], pos_w_lines=pwl, inv_level_sigma_sq_lsd=self.inv_sigma_sq_lsd, line_counts=frame["kl_counts"])
        self.mt.pose_optimize_device(self.camera, self.setup_type, B, cap, pose_in, v, frame["kps"], pw, self.inv_sigma_sq, {k: t for k, t in o.items() if t.numel()},
                                     x_right=frame.get("x_right"), counts=frame["counts"], num_trials=self.num_trials, num_each_iter=self.num_each_iter,
                                     pose_stride=pose_in.shape[1], stream=st, **kw)
        o.update(valid=v, pos_w=pw, valid_lines=vl, pos_w_lines=pwl)
        return o

    def run(self, frame, last, local, pose_pred, stream=None):
        """Enqueue the whole chain for the B frames.  Returns dict(last: the results of run_last_frame, opt1: the first optimiser's outputs (status,
        pose [B, 15], num_init_obs, num_valid, outlier, outlier_lines, trial_info, trial_chi2) with its inputs valid / pos_w / valid_lines /
        pos_w_lines, local: the results of run_local, opt2: the second optimiser's, pose [B, 15]: the optimised frame_pose rows, num_tracked /
        num_tracked_lines [B] i32, landmark / landmark_lines [B, cap]: the row each slot holds at the end (>= 0 into `last`, -2 - row into
        `local`, -1 none))."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        r1 = self.posed.run_last_frame(frame, last, pose_pred, stream=st)
        with torch.cuda.stream(st):
            v1, pw1, q1 = self.gather(r1["m1"], frame["counts"], last, "pos_w", "erased")
            vl1, pwl1, ql1 = self.gather(r1["m3"], frame["kl_counts"], last, "plucker_lines", "erased_lines")
        o1 = self._optimize("o1", frame, pose_pred, v1, pw1, vl1, pwl1, st)
        with torch.cuda.stream(st):
            # discard_outliers[_line]: landmarks_[idx] = nullptr where the flag is set (a landmark that will be erased keeps its slot: it was no edge)
            h1 = self._hit(r1["m1"], frame["counts"], last["pos_w"].shape[1]) & (o1["outlier"] == 0)
            hl1 = self._hit(r1["m3"], frame["kl_counts"], last["pos_w_lines"].shape[1])
            if self.use_lines:
                hl1 = hl1 & (o1["outlier_lines"] == 0)
            occ = self._has_obs(h1, q1, last.get("has_obs"))
            occ_l = self._has_obs(hl1, ql1, last.get("has_obs_lines"))
        r2 = self.posed.run_local(frame, local, o1["pose"], occ, occ_l, stream=st)
        with torch.cuda.stream(st):
            v2, pw2, q2 = self.gather(r2["m2"], frame["counts"], local, "pos_w", "erased")
            vl2, pwl2, ql2 = self.gather(r2["m4"], frame["kl_counts"], local, "plucker_lines", "erased_lines")
            g2 = self._hit(r2["m2"], frame["counts"], local["pos_w"].shape[1])
            gl2 = self._hit(r2["m4"], frame["kl_counts"], local["pos_w_lines"].shape[1])
            keep = h1 & ~g2
            keep_l = hl1 & ~gl2
            valid = v2 | (keep & v1)
            pos = torch.where(g2[..., None], pw2, pw1)
            valid_l = vl2 | (keep_l & vl1)
            pos_l = torch.where(gl2[..., None], pwl2, pwl1)
            lm = torch.where(g2, -2 - q2, torch.where(keep, q1, torch.full_like(q1, -1)))
            lm_l = torch.where(gl2, -2 - ql2, torch.where(keep_l, ql1, torch.full_like(ql1, -1)))
        o2 = self._optimize("o2", frame, o1["pose"], valid, pos, valid_l, pos_l, st)
        with torch.cuda.stream(st):
            tracked = ((lm != -1) & (o2["outlier"] == 0)).sum(1).to(torch.int32)
            tracked_l = ((lm_l != -1) & (o2["outlier_lines"] == 0)).sum(1).to(torch.int32) if self.use_lines else (lm_l != -1).sum(1).to(torch.int32)
        return dict(last=r1, opt1=o1, local=r2, opt2=o2, pose=o2["pose"], num_tracked=tracked, num_tracked_lines=tracked_l, landmark=lm, landmark_lines=lm_l)

    def _has_obs(self, hit, q, has_obs):
        torch = self.torch
        if has_obs is None or has_obs.shape[1] == 0:
            return hit.to(torch.uint8)
        return (hit & (torch.gather(has_obs, 1, q) != 0)).to(torch.uint8)
