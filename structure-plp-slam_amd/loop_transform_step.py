"""Sim3 refinement and the decision for the C loop candidates of one key frame: the solver's Sim3 and the mutual match in, the selected candidate
and its Sim3_world_to_curr out, on one stream, without the host.

For a current key frame (1) and C candidate key frames (2), `loop_transform_step.run` does what loop_detector::select_loop_candidate_via_Sim3
(module/loop_detector.cc:334-410) does per candidate after match_keyframes_mutually:

  1  torch, on the stream            the loop of transform_optimizer::optimize (optimize/transform_optimizer.cc:86-127) in slot form: for every key
                                     point idx1 of the current key frame the matched key point idx2 of the candidate, the two landmark rows, their
                                     `valid` byte, positions and key points.  A candidate whose Sim3 status is not SIM3_OK gets valid = 0 (the
                                     reference `continue`s at :371-374 before it reaches the optimiser)
  2  plp_transform_optimize_device   transform_optimizer_.optimize(cur, candidate, matches, g2o_sim3_cand_to_curr, 10)            :390-391
  3  torch, on the stream            accepted[c] = the solver found a Sim3 and num_optimized_inliers >= 20 (:394); selected = the lowest accepted c
                                     (the loop returns at the first one, :398-406) or -1; that candidate's g2o_Sim3_world_to_curr (:404)

Steps 1 and 3 are gathers of static shape (no .item(), no copy to the host, no boolean-mask indexing).  The input is what loop_sim3_step.run
returns (status, rot_12, trans_12, scale_12, pose_1) plus idx2, the match after the mutual search; the two FUSE | NO_CHI2 calls and the cross
check that produce idx2 are the caller's.

  valid[c][idx1] = idx2 >= 0 (:95), both key points carry a landmark (:104), neither landmark will_be_erased (:108).
                   lm_2->get_index_in_keyframe(keyfrm_2) (:113-118) is idx2 by construction: lm_2 is the landmark of key point idx2.

Tensors on the step's device:
  status [C] u8, rot_12 [C, 3, 3] f64, trans_12 [C, 3] f64, scale_12 [C] f32, pose_1 [C, 15] or [15] f64     loop_sim3_step.run's output
  pose_2 [C, 15] f64                                       the candidates' pose rows
  idx2 [C, cap1] i32                                       the matched key point of the candidate, -1 = none
  cur_kp [cap1, KP] u8, cand_kp [C, cap2, KP] u8           undist_keypts_ as rows of plp.KP_DTYPE bytes
  cur_lm [cap1] i32, cand_lm [C, cap2] i32                 key point -> landmark row, -1 = none
  pos_w [L, 3] f64, erased [L] u8                          the landmark table
"""
import numpy as np


class loop_transform_step:
    def __init__(self, plp, camera, inv_level_sigma_sq, fix_scale=False, num_iter=10, chi_sq=10.0, min_num_inliers=20, device_index=0, mt=None):
        """camera: a plp.camera_model; inv_level_sigma_sq: the key frames' inv_level_sigma_sq_ (host, num_levels floats); the defaults are the loop
        detector's (module/loop_detector.cc:390-394)"""
        import torch
        self.torch, self.plp, self.camera = torch, plp, camera
        self.dev = torch.device("cuda", device_index)
        self.sigma = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
        self.fix_scale, self.num_iter, self.chi_sq, self.min_num_inliers = bool(fix_scale), int(num_iter), float(chi_sq), int(min_num_inliers)
        self.mt = mt or plp.matcher(device=device_index)

    def gather(self, status, idx2, cur_kp, cand_kp, cur_lm, cand_lm, pos_w, erased):
        """step 1 on the current stream: dict(valid [C, cap1] u8, pos_w_1 / pos_w_2 [C, cap1, 3] f64, undist_1 / undist_2 [C, cap1, KP] u8)"""
        torch = self.torch
        i64 = torch.int64
        C, cap1 = idx2.shape
        cap2, L, KP = cand_lm.shape[1], pos_w.shape[0], cur_kp.shape[-1]
        t = idx2.to(i64)
        has = (t >= 0) & (t < cap2)
        t_c = t.clamp(0, max(cap2 - 1, 0))
        lm1 = cur_lm.to(i64).unsqueeze(0).expand(C, cap1)
        lm2 = torch.where(has, cand_lm.to(i64).gather(1, t_c), torch.full_like(t, -1))
        inside = has & (lm1 >= 0) & (lm1 < L) & (lm2 >= 0) & (lm2 < L)
        l1, l2 = lm1.clamp(0, L - 1), lm2.clamp(0, L - 1)
        er = erased.to(i64)
        solved = (status.to(i64) == self.plp.SIM3_OK).unsqueeze(1)
        valid = (solved & inside & (er[l1] == 0) & (er[l2] == 0)).to(torch.uint8).contiguous()
        return dict(valid=valid, pos_w_1=pos_w[l1].contiguous(), pos_w_2=pos_w[l2].contiguous(), undist_1=cur_kp.unsqueeze(0).expand(C, cap1, KP).contiguous(),
                    undist_2=cand_kp.gather(1, t_c.unsqueeze(2).expand(C, cap1, KP)).contiguous())

    def run(self, sim3, pose_2, idx2, cur_kp, cand_kp, cur_lm, cand_lm, pos_w, erased, stream=None):
        """Enqueue the three steps on `stream` (default: the current stream).  sim3: loop_sim3_step.run's output (status, rot_12, trans_12, scale_12,
        pose_1 are read).  Returns the gathered inputs and dict(the outputs of plp_transform_optimize_device named as in TRANSFORM_OPT_OUTPUTS,
        accepted [C] u8, selected [] i32: the lowest accepted candidate or -1, sim3_world_to_curr [13] f64: rot (9), trans (3), scale of the selected
        candidate, zeros when none is).  Nothing is synchronised."""
        torch, plp = self.torch, self.plp
        st = stream or torch.cuda.current_stream(self.dev)
        C, cap1 = idx2.shape
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
        with torch.cuda.stream(st):
            g = self.gather(sim3["status"], idx2, cur_kp, cand_kp, cur_lm, cand_lm, pos_w, erased)
            p1 = sim3["pose_1"].reshape(-1, 15).expand(C, 15).contiguous()
            rot = sim3["rot_12"].reshape(C, 9).contiguous()
            p2, trans, scale = pose_2.contiguous(), sim3["trans_12"].contiguous(), sim3["scale_12"].contiguous()     # a copy, if one is needed, belongs to `st`
            out = {k: torch.zeros((C,) + shape(cap1), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in plp.TRANSFORM_OPT_OUTPUTS.items()}
        if C:
            self.mt.transform_optimize_device(self.camera, self.fix_scale, C, cap1, g["valid"], g["pos_w_1"], g["pos_w_2"], g["undist_1"], g["undist_2"], p1,
                                              p2, rot, trans, scale, self.sigma, self.sigma,
                                              {k: v for k, v in out.items() if v.numel()}, num_iter=self.num_iter, chi_sq=self.chi_sq, stream=st)
        with torch.cuda.stream(st):
            accepted = (sim3["status"].to(torch.int64) == plp.SIM3_OK) & (out["num_inliers"] >= self.min_num_inliers)
            c = torch.arange(C, dtype=torch.int64, device=self.dev)
            first = torch.where(accepted, c, torch.full_like(c, C)).min() if C else torch.zeros((), dtype=torch.int64, device=self.dev)
            found = first < C
            row = torch.cat([out["world_to_1"], torch.zeros((1, 13), dtype=torch.float64, device=self.dev)]).index_select(0, first.clamp(0, C).reshape(1))[0]
            out.update(g, pose_1=p1, accepted=accepted.to(torch.uint8), selected=torch.where(found, first, torch.full_like(first, -1)).to(torch.int32),
                       sim3_world_to_curr=row)
        return out
