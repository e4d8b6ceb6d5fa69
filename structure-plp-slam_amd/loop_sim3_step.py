"""Sim3 estimation for the C loop candidates of one key frame: BoW matches and map tables in, a Sim3 and its inlier mask per candidate out, on
one stream, without the host.

For a current key frame (1) and C candidate key frames (2) whose key points, landmark rows and poses are already in HBM,
`loop_sim3_step.run` does what loop_detector::select_loop_candidate_via_Sim3 (module/loop_detector.cc:334-410) does per candidate between
its BoW match and its mutual projection match:

  1  torch, on the stream         the loop of sim3_solver's constructor (solve/sim3_solver.cc:70-115) in slot form: for every key point idx1 of
                                  the current key frame the matched key point idx2 of the candidate, the two landmark rows, their `valid` byte,
                                  positions and octaves
  2  plp_sim3_ransac_device       the constructor's arithmetic and find_via_ransac(iters)            status, rot_12, trans_12, scale_12, inliers

Step 1 is gathers and one scatter of static shape (no .item(), no copy to the host, no boolean-mask indexing).  Its input is the out_match
of a PLP_MATCH_MODE_BOW call with the candidate's key points as targets and the current key frame's key points as queries in BoW node order
(bow_tree::match_keyframes): out_match[c][idx2] = the query matched to key point idx2 of candidate c, q_feature[c][q] = the key point idx1
that query q is.  The match is one to one, so the scatter to idx1 has no collisions.

  valid[c][idx1] = a query was matched to some idx2 (:72), both key points carry a landmark (:80), neither landmark will_be_erased (:84).
                   lm_2->get_index_in_keyframe(keyfrm_2) (:89-94) is idx2 by construction: lm_2 is the landmark of key point idx2.

The outputs stay in HBM: rot_12 / trans_12 / scale_12 of a candidate whose status is SIM3_OK are what plp.mutual_poses turns into the pose
rows of plp_project_landmarks_* (INTEGRATION.md section 3); the optimiser that follows (optimize::transform_optimizer) stays on the host.

Tensors on the step's device:
  out_match [C, cap2] i32, q_feature [C, m_cap] i32        the BoW match
  cur_lm [cap1] i32, cand_lm [C, cap2] i32                 key point -> landmark row, -1 = none
  cur_octave [cap1] i32, cand_octave [C, cap2] i32         undist_keypts_[i].octave
  pos_w [L, 3] f64, erased [L] u8                          the landmark table
  pose_1 [15] f64, pose_2 [C, 15] f64                      the pose rows (entries 0-11 are read)
"""
import numpy as np


class loop_sim3_step:
    def __init__(self, plp, camera, level_sigma_sq, fix_scale=False, min_num_inliers=20, iters=200, device_index=0, mt=None):
        """camera: a plp.camera_model; level_sigma_sq: the key frames' level_sigma_sq_ (host, num_levels floats); the defaults are the loop
        detector's (module/loop_detector.cc:370-371)"""
        import torch
        self.torch, self.plp, self.camera = torch, plp, camera
        self.dev = torch.device("cuda", device_index)
        self.sigma = np.ascontiguousarray(level_sigma_sq, np.float32).reshape(-1)
        self.fix_scale, self.min_num_inliers, self.iters = bool(fix_scale), int(min_num_inliers), int(iters)
        self.mt = mt or plp.matcher(device=device_index)

    def gather(self, out_match, q_feature, cur_lm, cand_lm, cur_octave, cand_octave, pos_w, erased):
        """step 1 on the current stream: dict(valid [C, cap1] u8, pos_w_1 / pos_w_2 [C, cap1, 3] f64, octave_1 / octave_2 [C, cap1] i32, idx2
        [C, cap1] i32: the matched key point of the candidate, -1 = none)"""
        torch = self.torch
        i64 = torch.int64
        C, cap2 = out_match.shape
        cap1, L = cur_lm.shape[0], pos_w.shape[0]
        q = out_match.to(i64)
        hit = (q >= 0) & (q < q_feature.shape[1])
        idx1 = q_feature.to(i64).gather(1, q.clamp(0, q_feature.shape[1] - 1))
        hit = hit & (idx1 >= 0) & (idx1 < cap1)
        t = torch.arange(cap2, dtype=i64, device=self.dev).unsqueeze(0).expand(C, cap2)
        idx2 = torch.full((C, cap1 + 1), -1, dtype=i64, device=self.dev)          # column cap1 takes the key points without a match
        idx2.scatter_(1, torch.where(hit, idx1, torch.full_like(idx1, cap1)), torch.where(hit, t, torch.full_like(t, -1)))
        idx2 = idx2[:, :cap1]
        has = idx2 >= 0
        t_c = idx2.clamp(0, cap2 - 1)
        lm1 = cur_lm.to(i64).unsqueeze(0).expand(C, cap1)
        lm2 = torch.where(has, cand_lm.to(i64).gather(1, t_c), torch.full_like(idx2, -1))
        inside = has & (lm1 >= 0) & (lm1 < L) & (lm2 >= 0) & (lm2 < L)
        l1, l2 = lm1.clamp(0, L - 1), lm2.clamp(0, L - 1)
        er = erased.to(i64)
        valid = (inside & (er[l1] == 0) & (er[l2] == 0)).to(torch.uint8).contiguous()
        return dict(valid=valid, pos_w_1=pos_w[l1].contiguous(), pos_w_2=pos_w[l2].contiguous(),
                    octave_1=cur_octave.to(torch.int32).unsqueeze(0).expand(C, cap1).contiguous(),
                    octave_2=cand_octave.to(i64).gather(1, t_c).to(torch.int32).contiguous(), idx2=idx2.to(torch.int32))

    def run(self, out_match, q_feature, cur_lm, cand_lm, cur_octave, cand_octave, pos_w, erased, pose_1, pose_2, samples=None, seed=0, stream=None):
        """Enqueue both steps on `stream` (default: the current stream).  Returns the gathered inputs and dict(status [C] u8, num_common,
        num_inliers, best_iter [C] i32, rot_12 [C, 3, 3], trans_12 [C, 3] f64, scale_12 [C] f32, inliers [C, cap1] u8 per key point of the current
        key frame).  samples [C, iters, 3] i32 or None = drawn from seed.  Nothing is synchronised."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        C, cap1 = out_match.shape[0], cur_lm.shape[0]
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
        with torch.cuda.stream(st):
            g = self.gather(out_match, q_feature, cur_lm, cand_lm, cur_octave, cand_octave, pos_w, erased)
            p1 = pose_1.reshape(1, 15).expand(C, 15).contiguous()
            out = {k: torch.zeros((C,) + shape(cap1, self.iters), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in self.plp.SIM3_OUTPUTS.items()
                   if k != "hyp_inliers"}
        if C and cap1:
            self.mt.sim3_ransac_device(self.camera, C, cap1, g["valid"], g["pos_w_1"], g["pos_w_2"], g["octave_1"], g["octave_2"], p1, pose_2.contiguous(),
                                       self.sigma, self.sigma, out, iters=self.iters, fix_scale=self.fix_scale, min_num_inliers=self.min_num_inliers,
                                       samples=samples, seed=seed, stream=st)
        out.update(g, pose_1=p1)
        return out
