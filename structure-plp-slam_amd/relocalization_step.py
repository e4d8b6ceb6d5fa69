"""EPnP + RANSAC for the C relocalisation candidates of one frame: BoW matches and map tables in, a pose and its inlier mask per candidate
out, on one stream, without the host.

For a frame whose bearings and octaves are in HBM and C candidate key frames whose landmark rows are, `relocalization_step.run` does what
module::relocalizer::relocalize (module/relocalizer.cc:55-252) does per candidate between its BoW match (:79) and its pose optimiser (:118):

  1  torch, on the stream         extract_valid_indices + setup_pnp_solver (relocalizer.cc:254-291) in slot form: for every key point of the
                                  frame the landmark row matched to it, its `valid` byte and position; the frame's bearing and octave
  2  plp_pnp_ransac_device        the constructor's thresholds and find_via_ransac(iters) (:93)      status, rot_cw, trans_cw, inliers
  3  torch, on the stream         the 15-double pose row plp_project_landmarks_* takes (frame::update_pose_params, :99-100)

Steps 1 and 3 are gathers and elementwise arithmetic of static shape (no .item(), no copy to the host, no boolean-mask indexing).  The input
of step 1 is the out_match of a PLP_MATCH_MODE_BOW call with the frame's key points as targets and the candidate's key points that carry a
live landmark as queries in BoW node order (bow_tree::match_frame_and_keyframe): out_match[c][idx] = the query matched to key point idx of
the frame, q_feature[c][q] = the key point of candidate c that query q is.  matched_landmarks.at(idx) is that key point's landmark.

  valid[c][idx] = a query was matched to idx (relocalizer.cc:261) whose landmark will not be erased (:265)

The outputs stay in HBM: the pose row of a candidate whose status is PNP_OK is the `pose` of the projection match that follows
(projection::match_frame_and_keyframe, :137), its inlier mask selects the landmarks the pose optimiser starts from
(:104-115).  optimize::pose_optimizer (g2o) and everything on keyframe objects stay on the host.

Tensors on the step's device:
  out_match [C, cap] i32, q_feature [C, m_cap] i32         the BoW match
  cand_lm [C, cap2] i32                                    key point of the candidate -> landmark row, -1 = none
  bearing [cap, 3] f64, octave [cap] i32                   curr_frm.bearings_, curr_frm.keypts_[i].octave
  pos_w [L, 3] f64, erased [L] u8                          the landmark table
"""
import numpy as np


class relocalization_step:
    def __init__(self, plp, scale_factors, min_num_inliers=10, iters=30, recompute=True, device_index=0, mt=None):
        """scale_factors: the frame's scale_factors_ (host, num_levels floats); the defaults are the relocaliser's (module/relocalizer.cc:93,
        solve/pnp_solver.h)"""
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.scale_factors = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        self.min_num_inliers, self.iters, self.recompute = int(min_num_inliers), int(iters), bool(recompute)
        self.mt = mt or plp.matcher(device=device_index)

    def gather(self, out_match, q_feature, cand_lm, bearing, octave, pos_w, erased):
        """step 1 on the current stream: dict(valid [C, cap] u8, bearing / pos_w [C, cap, 3] f64, octave [C, cap] i32, landmark [C, cap] i32:
        the matched landmark row, -1 = none)"""
        torch = self.torch
        i64 = torch.int64
        C, cap = out_match.shape
        m_cap, cap2, L = q_feature.shape[1], cand_lm.shape[1], pos_w.shape[0]
        q = out_match.to(i64)
        hit = (q >= 0) & (q < m_cap)
        kp2 = q_feature.to(i64).gather(1, q.clamp(0, max(m_cap - 1, 0)))
        hit = hit & (kp2 >= 0) & (kp2 < cap2)
        lm = cand_lm.to(i64).gather(1, kp2.clamp(0, max(cap2 - 1, 0)))
        inside = hit & (lm >= 0) & (lm < L)
        row = lm.clamp(0, max(L - 1, 0))
        valid = (inside & (erased.to(i64)[row] == 0)).to(torch.uint8).contiguous()
        return dict(valid=valid, pos_w=pos_w[row].contiguous(), bearing=bearing.unsqueeze(0).expand(C, cap, 3).contiguous(),
                    octave=octave.to(torch.int32).unsqueeze(0).expand(C, cap).contiguous(),
                    landmark=torch.where(inside, lm, torch.full_like(lm, -1)).to(torch.int32))

    def pose_rows(self, rot_cw, trans_cw):
        """step 3: [C, 15] f64 -- rot_cw row-major, trans_cw and cam_center = -rot_cw^T trans_cw formed as plp.frame_pose forms it (each
        coefficient a left-to-right sum of the negated column times trans_cw)"""
        torch = self.torch
        R, t = rot_cw, trans_cw
        cc = [((-R[:, 0, i]) * t[:, 0] + (-R[:, 1, i]) * t[:, 1]) + (-R[:, 2, i]) * t[:, 2] for i in range(3)]
        return torch.cat([R.reshape(-1, 9), t, torch.stack(cc, 1)], 1).contiguous()

    def run(self, out_match, q_feature, cand_lm, bearing, octave, pos_w, erased, samples=None, seed=0, stream=None):
        """Enqueue the three steps on `stream` (default: the current stream).  Returns the gathered inputs and dict(status [C] u8, num_matches,
        num_inliers, best_iter [C] i32, rot_cw [C, 3, 3], trans_cw [C, 3] f64, inliers [C, cap] u8 per key point of the frame, pose [C, 15]
        f64; rot_cw, trans_cw, inliers and pose are zero and best_iter is -1 unless the status is PNP_OK).  samples [C, iters, 4] i32 or None = drawn from seed.  Nothing is synchronised."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        C, cap = out_match.shape
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
        with torch.cuda.stream(st):
            g = self.gather(out_match, q_feature, cand_lm, bearing, octave, pos_w, erased)
            out = {k: torch.zeros((C,) + shape(cap, self.iters), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in self.plp.PNP_OUTPUTS.items()
                   if k != "hyp_inliers"}
        if C and cap:
            self.mt.pnp_ransac_device(C, cap, g["valid"], g["bearing"], g["pos_w"], g["octave"], self.scale_factors, out, iters=self.iters,
                                      min_num_inliers=self.min_num_inliers, recompute=self.recompute, samples=samples, seed=seed, stream=st)
        with torch.cuda.stream(st):
            out["pose"] = self.pose_rows(out["rot_cw"], out["trans_cw"])
        out.update({k: v for k, v in g.items() if k not in out})
        return out
