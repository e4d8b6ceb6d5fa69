"""The monocular map initialisation of B pairs of frames on one stream, without the host: initialize::bearing_vector::initialize, and the inlier
filter of match::robust::match_frame_and_keyframe.

For B pairs (reference frame 1, current frame 2) whose bearings are in HBM as the post-extract step leaves them and whose matches are the
out_match of a plp_match_* call (slot = key point of frame 1, value = key point of frame 2 or a negative number), the step runs
plp_essential_ransac_device and plp_two_view_pose_device and returns their outputs as tensors that stay in HBM:

  initializer_step.run(...)            initialize::bearing_vector::initialize (initialize/bearing_vector.cc:48-107): find_via_ransac(100), then
                                       plp_two_view_pose_device -- essential_solver::decompose and find_most_plausible_pose with its four
                                       check_pose calls (initialize/base.cc:62-243) -- on the RANSAC's outputs where they lie: status, the pose
                                       ref -> cur, the triangulated points and their flags per key point of frame 1, from which
                                       module::initializer::create_map_for_monocular builds its key frames and landmarks.
  initializer_step.essential(...)      the RANSAC alone: status, E_21, score, the inlier mask per key point of frame 1.
  initializer_step.robust_inliers(...) find_via_ransac(50, false) of match::robust::match_frame_and_keyframe (match/robust.cc:231-254): the
                                       mask of the brute-force matches it keeps and their number, zero matches where the solution is not
                                       valid (:234-237).  matched_lms_in_frm is the caller's gather of the key frame's landmarks under the
                                       mask (:241-252): lm[b][idx1] = mask[b][idx1] ? keyfrm_lms[b][match[b][idx1]] : none.

Tensors on the step's device:
  bearing_1 [B, n_cap, 3] f64, bearing_2 [B, m_cap, 3] f64       frame::bearings_ of both frames
  match [B, n_cap] i32                                            the matcher's out_match
  counts_1 / counts_2 [B] i32 or None                             key points in use
"""
import numpy as np


class initializer_step:
    def __init__(self, plp, num_ransac_iters=100, device_index=0, mt=None):
        """num_ransac_iters: initialize::base's num_ransac_iters_ (100 by module/initializer.cc's default)"""
        import torch
        self.torch, self.plp = torch, plp
        self.dev = torch.device("cuda", device_index)
        self.num_ransac_iters = int(num_ransac_iters)
        self.mt = mt or plp.matcher(device=device_index)

    def _ransac(self, bearing_1, bearing_2, match, iters, recompute, counts_1, counts_2, samples, seed, stream):
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        B, n_cap = match.shape
        m_cap = bearing_2.shape[1]
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
        with torch.cuda.stream(st):
            out = {k: torch.zeros((B,) + shape(n_cap, iters), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in self.plp.ESSENTIAL_OUTPUTS.items()
                   if k != "hyp_score"}
            if B and n_cap:
                out["status"].fill_(self.plp.ESSENTIAL_TOO_FEW_MATCHES)   # a pair the entry does not reach (m_cap == 0) has no match
                out["best_iter"].fill_(-1)
        if B and n_cap and m_cap:
            self.mt.essential_ransac_device(B, n_cap, m_cap, bearing_1.contiguous(), bearing_2.contiguous(), match.contiguous(), out, iters=iters,
                                            recompute=recompute, samples=samples, seed=seed, counts_1=counts_1, counts_2=counts_2, stream=st)
        return out

    def run(self, camera, bearing_1, bearing_2, match, undist_1, undist_2, counts_1=None, counts_2=None, samples=None, seed=0, min_num_triangulated=50,
            parallax_deg_thr=1.0, reproj_err_thr=4.0, img_bounds=None, stream=None):
        """Enqueue initialize::bearing_vector::initialize of B (reference, current) pairs on `stream` (default: the current stream):
        plp_essential_ransac_device (num_ransac_iters, refit) -> plp_two_view_pose_device, the second reading the first's status, matrix and mask in
        HBM.  camera: a camera_model; undist_1 [B, n_cap] / undist_2 [B, m_cap]: the post-extract step's undistorted key points (plp_keypoint rows,
        any tensor of 28 bytes per key point).  Returns dict(status [B] u8: TWO_VIEW_*, rot_ref_to_cur [B, 3, 3], trans_ref_to_cur [B, 3] f64,
        hypothesis [B] i32, num_valid [B, 4] i32, parallax_deg [B, 4] f32, triangulated_pts [B, n_cap, 3] f64, is_triangulated [B, n_cap] u8 --
        the arrays from which module::initializer::create_map_for_monocular builds its two key frames and its landmarks; zero unless the status is
        TWO_VIEW_OK -- and essential: the RANSAC's outputs).  Nothing is synchronised; the object creation, scale_map and the global adjustment stay
        with the caller."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        e = self.essential(bearing_1, bearing_2, match, counts_1, counts_2, samples, seed, st)
        B, n_cap = match.shape
        m_cap = bearing_2.shape[1]
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
        with torch.cuda.stream(st):
            out = {k: torch.zeros((B,) + shape(n_cap), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in self.plp.TWO_VIEW_OUTPUTS.items()
                   if k != "hyp_is_triangulated"}
            if B and n_cap:
                out["status"].fill_(self.plp.TWO_VIEW_NO_SOLUTION)
                out["hypothesis"].fill_(-1)
        if B and n_cap and m_cap:
            self.mt.two_view_pose_device(camera, B, n_cap, m_cap, e["E_21"], e["inliers"], match.contiguous(), bearing_1.contiguous(), bearing_2.contiguous(),
                                         undist_1.contiguous(), undist_2.contiguous(), out, min_num_triangulated=min_num_triangulated,
                                         parallax_deg_thr=parallax_deg_thr, reproj_err_thr=reproj_err_thr, depth_is_positive=False, in_status=e["status"],
                                         counts_1=counts_1, counts_2=counts_2, img_bounds=img_bounds, stream=st)
        out["essential"] = e
        return out

    def essential(self, bearing_1, bearing_2, match, counts_1=None, counts_2=None, samples=None, seed=0, stream=None):
        """Enqueue find_via_ransac(num_ransac_iters) of B pairs on `stream` (default: the current stream).  Returns dict(status [B] u8:
        ESSENTIAL_*, num_matches, num_inliers, best_iter [B] i32, E_21 [B, 3, 3] f64, score [B] f32, inliers [B, n_cap] u8 per key point of
        frame 1; E_21, score, num_inliers and inliers are zero and best_iter is -1 unless the status is ESSENTIAL_OK).  samples
        [B, num_ransac_iters, 8] i32 or None = drawn from seed.  Nothing is synchronised."""
        return self._ransac(bearing_1, bearing_2, match, self.num_ransac_iters, True, counts_1, counts_2, samples, seed, stream)

    def robust_inliers(self, bearing_1, bearing_2, match, counts_1=None, counts_2=None, samples=None, seed=0, stream=None):
        """Enqueue find_via_ransac(50, false) of B (frame, key frame) pairs.  Returns dict(inliers [B, n_cap] u8: the matches
        robust::match_frame_and_keyframe keeps, per key point of the frame; num_inlier_matches [B] i32: what it returns, 0 where the solution is
        not valid; status [B] u8).  samples [B, 50, 8] i32 or None = drawn from seed.  Nothing is synchronised."""
        out = self._ransac(bearing_1, bearing_2, match, 50, False, counts_1, counts_2, samples, seed, stream)
        return dict(inliers=out["inliers"], num_inlier_matches=out["num_inliers"], status=out["status"])

    def run_perspective(self, camera, bearing_1, bearing_2, match, undist_1, undist_2, counts_1=None, counts_2=None, samples_h=None, samples_f=None, seed=0,
                        given_H_21=None, given_H_num_inliers=None, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, img_bounds=None, stream=None):
        """Enqueue initialize::perspective::initialize (initialize/perspective.cc:48-174) of B (reference, current) pairs on `stream` (default: the
        current stream): homography_fundamental(...) -> plp_perspective_pose_device, the second reading the first's choice, matrices and mask in HBM
        (DESIGN.md section 5, D27).  camera: a camera_model of the perspective or fisheye model.  Returns the tensors named as
        PERSPECTIVE_POSE_OUTPUTS without the per-hypothesis flags (status [B] u8: TWO_VIEW_* or PERSPECTIVE_POSE_NO_DECOMPOSITION, the pose ref -> cur,
        hypothesis, num_valid / parallax_deg [B, 8], triangulated_pts [B, n_cap, 3], is_triangulated [B, n_cap]) and ransac: the solvers' outputs.
        Nothing is synchronised; the object creation and scale_map stay with the caller."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        e = self.homography_fundamental(undist_1, undist_2, match, counts_1, counts_2, samples_h, samples_f, seed, given_H_21, given_H_num_inliers, st)
        B, n_cap = match.shape
        m_cap = bearing_2.shape[1]
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
        with torch.cuda.stream(st):
            out = {k: torch.zeros((B,) + shape(n_cap), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in self.plp.PERSPECTIVE_POSE_OUTPUTS.items()
                   if k != "hyp_is_triangulated"}
            if B and n_cap:
                out["status"].fill_(self.plp.TWO_VIEW_NO_SOLUTION)
                out["hypothesis"].fill_(-1)
        if B and n_cap and m_cap:
            self.mt.perspective_pose_device(camera, B, n_cap, m_cap, e["choice"], e["H_21"], e["F_21"], e["inliers"], match.contiguous(), bearing_1.contiguous(),
                                            bearing_2.contiguous(), undist_1.contiguous(), undist_2.contiguous(), out, min_num_triangulated=min_num_triangulated,
                                            parallax_deg_thr=parallax_deg_thr, reproj_err_thr=reproj_err_thr, counts_1=counts_1, counts_2=counts_2,
                                            img_bounds=img_bounds, stream=st)
        out["ransac"] = e
        return out

    def homography_fundamental(self, undist_1, undist_2, match, counts_1=None, counts_2=None, samples_h=None, samples_f=None, seed=0, given_H_21=None,
                               given_H_num_inliers=None, stream=None):
        """Enqueue the two solvers of initialize::perspective::initialize (initialize/perspective.cc:84-120) and the choice between them for B pairs
        on `stream` (default: the current stream): plp_perspective_ransac_device with num_ransac_iters hypotheses per
        solver and the refit.  undist_1 [B, n_cap] / undist_2 [B, m_cap]: the post-extract step's undistorted key points (plp_keypoint rows, any
        tensor of 28 bytes per key point); samples_h / samples_f [B, num_ransac_iters, 8] i32 or None = drawn from seed; given_H_21 [B, 3, 3] f64
        with given_H_num_inliers [B] i32: the homography of the caller's graph-cut RANSAC for the pairs whose count is not negative, which then
        run no H hypotheses.  Returns the tensors named as PERSPECTIVE_RANSAC_OUTPUTS without the per-hypothesis scores: status_h / status_f [B] u8
        PERSPECTIVE_*, choice [B] u8 PERSPECTIVE_CHOICE_*, H_21 / F_21 [B, 3, 3] f64, the scores, rel_score_h, and the inlier masks per key point
        of frame 1 (inliers: the chosen solver's).  Nothing is synchronised."""
        torch = self.torch
        st = stream or torch.cuda.current_stream(self.dev)
        B, n_cap = match.shape
        kp_bytes = self.plp.KP_DTYPE.itemsize
        m_cap = undist_2.numel() * undist_2.element_size() // (kp_bytes * B) if B else 0
        tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
        iters = self.num_ransac_iters
        with torch.cuda.stream(st):
            out = {k: torch.zeros((B,) + shape(n_cap, iters), dtype=tt[dt], device=self.dev) for k, (shape, dt, _) in self.plp.PERSPECTIVE_RANSAC_OUTPUTS.items()
                   if not k.startswith("hyp_score")}
        if B and n_cap:
            self.mt.perspective_ransac_device(B, n_cap, m_cap, undist_1.contiguous(), undist_2.contiguous() if m_cap else None, match.contiguous(), out, iters=iters,
                                              recompute=True, samples_h=samples_h, samples_f=samples_f, seed=seed, counts_1=counts_1, counts_2=counts_2,
                                              given_H_21=given_H_21, given_H_num_inliers=given_H_num_inliers, stream=st)
        return out
