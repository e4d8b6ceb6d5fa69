"""Map initialisation of the perspective and fisheye cameras: the two solvers of initialize::perspective::initialize and the choice between them
(include/plp_front.h: plp_perspective_ransac_*, the plp_model_* host builds of csrc/perspective_init.hpp): the numpy side of
the host-pointer entry and the host builds, and the mirror classes under the reference's names."""

import numpy as np

from ._abi import KP_DTYPE, PERSPECTIVE_OK, _struct, camera_model_c, perspective_pose_args_c, perspective_ransac_args_c
from ._core import PLP_ERR_INVALID_ARG, PlpError, lib
from ._marshal import array_or_none, host_ptr, host_ptrs, model_call, out_arrays, set_outputs, wanted

# the outputs of plp_perspective_ransac_*: name -> (shape per problem given (n_cap, iters), dtype, optional)
_ONE, _MAT = (lambda M, I: ()), (lambda M, I: (3, 3))
PERSPECTIVE_RANSAC_OUTPUTS = dict(
    status_h=(_ONE, np.uint8, False), status_f=(_ONE, np.uint8, False), num_matches=(_ONE, np.int32, False), H_21=(_MAT, np.float64, False),
    F_21=(_MAT, np.float64, False), score_h=(_ONE, np.float32, False), score_f=(_ONE, np.float32, False), best_iter_h=(_ONE, np.int32, False),
    best_iter_f=(_ONE, np.int32, False), num_inliers_h=(_ONE, np.int32, False), num_inliers_f=(_ONE, np.int32, False), rel_score_h=(_ONE, np.float32, False),
    choice=(_ONE, np.uint8, False), inliers=(lambda M, I: (M,), np.uint8, False), inliers_h=(lambda M, I: (M,), np.uint8, True),
    inliers_f=(lambda M, I: (M,), np.uint8, True), hyp_score_h=(lambda M, I: (I,), np.float32, True), hyp_score_f=(lambda M, I: (I,), np.float32, True))


def _keypoints(v):
    """key points as a KP_DTYPE array: a record array as it is, (..., 2) numbers as pt with the other fields zero"""
    a = np.asarray(v)
    if a.dtype == KP_DTYPE:
        return np.ascontiguousarray(a)
    a = np.asarray(a, np.float32)
    kp = np.zeros(a.shape[:-1], KP_DTYPE)
    kp["x"], kp["y"], kp["class_id"] = a[..., 0], a[..., 1], -1
    return kp


def _perspective_ransac_host(call, undist_1, undist_2, match, iters, recompute, samples_h, samples_f, seed, counts_1, counts_2, given_H_21, given_H_num_inliers,
                             outputs, out):
    """the numpy side of plp_perspective_ransac_host and plp_model_perspective_ransac_host: call(args struct) runs the entry"""
    ma = np.ascontiguousarray(match, np.int32)
    if ma.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "match must be (P, n_cap)")
    P_, M = ma.shape
    k1 = _keypoints(undist_1).reshape(P_, M)
    k2 = _keypoints(undist_2)
    k2 = k2.reshape(P_, -1) if P_ else k2.reshape(0, 0)
    I = int(iters)
    sh = None if samples_h is None else np.ascontiguousarray(samples_h, np.int32).reshape(P_, I, 8)
    sf = None if samples_f is None else np.ascontiguousarray(samples_f, np.int32).reshape(P_, I, 8)
    c1, c2 = array_or_none(counts_1, np.int32, P_), array_or_none(counts_2, np.int32, P_)
    gh, gn = array_or_none(given_H_21, np.float64, P_, 9), array_or_none(given_H_num_inliers, np.int32, P_)
    o = out_arrays(((k, (P_,) + shape(M, max(I, 0)), dt) for k, (shape, dt, optional) in PERSPECTIVE_RANSAC_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    a = _struct(perspective_ransac_args_c, dict(P=P_, n_cap=M, m_cap=k2.shape[1], iters=I, recompute=int(bool(recompute)), seed=int(seed) & 0xFFFFFFFFFFFFFFFF),
                host_ptrs(counts_1=c1, counts_2=c2, undist_1=k1, undist_2=k2, match=ma, samples_h=sh, samples_f=sf, given_H_21=gh, given_H_num_inliers=gn))
    set_outputs(a, PERSPECTIVE_RANSAC_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_perspective_ransac(undist_1, undist_2, match, iters=100, recompute=True, samples_h=None, samples_f=None, seed=0, counts_1=None, counts_2=None,
                             given_H_21=None, given_H_num_inliers=None, outputs=None, out=None):
    """Host build of the two solvers of initialize::perspective::initialize and the choice between them (csrc/perspective_init.hpp, DESIGN.md section
    5, D27; no GPU needed): the arguments and the result of matcher.perspective_ransac."""
    return _perspective_ransac_host(model_call("plp_model_perspective_ransac_host", "P"), undist_1, undist_2, match, iters, recompute, samples_h, samples_f, seed,
                                    counts_1, counts_2, given_H_21, given_H_num_inliers, outputs, out)


def model_normalize_keypoints(keypts):
    """Host build of solve::normalize (solve/common.cc:31-76; D27 item a; no GPU needed) of one frame's key points.  Returns dict(normalized (n, 2)
    f32, stats (4,) f32: mean_x, mean_y, 1 / dev_x, 1 / dev_y, transform (3, 3) f64)."""
    kp = _keypoints(keypts).reshape(-1)
    o = dict(normalized=np.zeros((len(kp), 2), np.float32), stats=np.zeros(4, np.float32), transform=np.zeros((3, 3)))
    if lib().plp_model_normalize_keypoints_host(host_ptr(kp), len(kp), host_ptr(o["normalized"]), host_ptr(o["stats"]), host_ptr(o["transform"])) != len(kp):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_normalize_keypoints_host")
    return o


def _model_fit(symbol, key, pts_1, pts_2, offsets):
    p1 = np.ascontiguousarray(pts_1, np.float32).reshape(-1, 2); p2 = np.ascontiguousarray(pts_2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise PlpError(PLP_ERR_INVALID_ARG, "pts_1 and pts_2 must hold the same number of rows")
    single = offsets is None
    off = np.array([0, len(p1)], np.int32) if single else np.ascontiguousarray(offsets, np.int32).reshape(-1)
    n = len(off) - 1
    if n < 0 or (n and int(off[-1]) > len(p1)):
        raise PlpError(PLP_ERR_INVALID_ARG, "offsets must be ascending within the rows")
    o = {key: np.zeros((n, 3, 3)), "sweeps": np.zeros(n, np.int32)}
    if getattr(lib(), symbol)(host_ptr(p1), host_ptr(p2), host_ptr(off), n, host_ptr(o[key]), host_ptr(o["sweeps"])) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "offsets must be ascending within the rows")
    return {k: v[0] for k, v in o.items()} if single else o


def model_homography_fit(pts_1, pts_2, offsets=None):
    """Host build of homography_solver::compute_H_21 (solve/homography_solver.cc:405-436; D27 item b; no GPU needed) for lists of point pairs: pts_1 /
    pts_2 (n_rows, 2) f32; list i holds rows offsets[i] .. offsets[i+1] (None: one list of all rows).  Returns dict(H_21 (n, 3, 3), sweeps (n,))."""
    return _model_fit("plp_model_homography_fit_host", "H_21", pts_1, pts_2, offsets)


def model_fundamental_fit(pts_1, pts_2, offsets=None):
    """Host build of fundamental_solver::compute_F_21 (solve/fundamental_solver.cc:299-332; D27 item b; no GPU needed); as model_homography_fit, F_21."""
    return _model_fit("plp_model_fundamental_fit_host", "F_21", pts_1, pts_2, offsets)


def _model_check(symbol, undist_1, undist_2, match, Ms):
    ma = np.ascontiguousarray(match, np.int32).reshape(-1)
    k1, k2 = _keypoints(undist_1).reshape(len(ma)), _keypoints(undist_2).reshape(-1)
    E = np.ascontiguousarray(Ms, np.float64)
    single = E.ndim == 2
    E = E.reshape(-1, 3, 3)
    n = len(E)
    o = dict(score=np.zeros(n, np.float32), num_inliers=np.zeros(n, np.int32), inliers=np.zeros((n, len(ma)), np.uint8))
    if getattr(lib(), symbol)(host_ptr(k1), host_ptr(k2), host_ptr(ma), len(ma), len(k2), host_ptr(E), n, host_ptr(o["score"]), host_ptr(o["num_inliers"]),
                              host_ptr(o["inliers"])) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, symbol)
    return {k: v[0] for k, v in o.items()} if single else o


def model_homography_check(undist_1, undist_2, match, H_21):
    """Host build of homography_solver::check_inliers (solve/homography_solver.cc:556-631; no GPU needed) of n matrices against one problem: key
    points of both frames, match (n_cap,), H_21 (n, 3, 3) or (3, 3).  Returns dict(score f32, num_inliers, inliers (n, n_cap) u8 in slot order)."""
    return _model_check("plp_model_homography_check_host", undist_1, undist_2, match, H_21)


def model_fundamental_check(undist_1, undist_2, match, F_21):
    """Host build of fundamental_solver::check_inliers (solve/fundamental_solver.cc:349-426; no GPU needed); as model_homography_check."""
    return _model_check("plp_model_fundamental_check_host", undist_1, undist_2, match, F_21)


def model_perspective_draw(solver, seed, p, iters, num_matches, iter0=0):
    """The samples plp_perspective_ransac_* draw for problem p when the caller passes none (D27 item f; no GPU needed); solver 0 = H, 1 = F: (iters, 8)"""
    out = np.zeros((int(iters), 8), np.int32)
    if lib().plp_model_perspective_draw_host(int(solver), int(seed) & 0xFFFFFFFFFFFFFFFF, int(p), int(iter0), int(iters), int(num_matches), host_ptr(out)) != int(iters):
        raise PlpError(PLP_ERR_INVALID_ARG, "num_matches must be at least 8, iters non-negative, solver 0 or 1")
    return out


class _perspective_solver:
    """What the two mirror classes share: undist_keypts_1 (n1) / undist_keypts_2 (n2) key points (records or (n, 2) points), matches_12 a list of
    (idx1, idx2) pairs in ascending idx1, every idx1 at most once.  mt: a matcher (the GPU entry), or None = the host build.  The entry runs both
    solvers; each class shows its own."""
    _S = None   # "h" or "f"

    def __init__(self, undist_keypts_1, undist_keypts_2, matches_12, sigma=1.0, mt=None, samples=None, seed=0):
        if float(sigma) != 1.0:
            raise PlpError(PLP_ERR_INVALID_ARG, "sigma is 1.0 (initialize/perspective.cc:84-87)")
        k1, k2 = _keypoints(undist_keypts_1).reshape(-1), _keypoints(undist_keypts_2).reshape(-1)
        m = np.asarray(matches_12, np.int64).reshape(-1, 2)
        if len(m) and (np.any(np.diff(m[:, 0]) <= 0) or m[:, 0].min() < 0 or m[:, 0].max() >= len(k1) or m[:, 1].min() < 0 or m[:, 1].max() >= len(k2)):
            raise PlpError(PLP_ERR_INVALID_ARG, "matches_12 must name key points of both frames, in strictly ascending idx1")
        match = np.full((1, max(len(k1), 1)), -1, np.int32)
        match[0, m[:, 0]] = m[:, 1]
        self._idx1 = m[:, 0].copy()
        pad = lambda k: k.reshape(1, -1) if len(k) else np.zeros((1, 1), KP_DTYPE)
        self._in = (pad(k1), pad(k2), match)
        self._kw = dict(seed=seed, counts_1=[len(k1)], counts_2=[len(k2)], **{"samples_" + self._S: samples})
        self._mt = mt
        self._r = None

    def _run(self, **kw):
        fn = model_perspective_ransac if self._mt is None else self._mt.perspective_ransac
        self._r = fn(*self._in, **self._kw, **kw)

    def find_via_ransac(self, max_num_iter, recompute=True):
        self._run(iters=int(max_num_iter), recompute=recompute)

    def solution_is_valid(self):
        return self._r is not None and int(self._r["status_" + self._S][0]) == PERSPECTIVE_OK

    def get_best_score(self):
        return float(self._r["score_" + self._S][0])

    def get_inlier_matches(self):
        """is_inlier_match_: one flag per match of matches_12, in its order"""
        return self._r["inliers_" + self._S][0, self._idx1].astype(bool)


class homography_solver(_perspective_solver):
    """Mirror of solve::homography_solver (solve/homography_solver.h)."""
    _S = "h"

    def use_matrix(self, H_21, num_inliers):
        """What find_via_graph_cut_ransac does once its RANSAC has a matrix and an inlier count (solve/homography_solver.cc:388-402)"""
        self._run(iters=1, recompute=False, given_H_21=np.asarray(H_21, np.float64).reshape(1, 9), given_H_num_inliers=[int(num_inliers)])

    def get_best_H_21(self):
        return self._r["H_21"][0].copy()

    @staticmethod
    def decompose(H_21, cam_matrix_1, cam_matrix_2=None):
        """homography_solver::decompose (solve/homography_solver.cc:438-554; static, as in the reference) of one matrix under the camera matrix of
        both frames (initialize::perspective passes the same one twice).  Returns (ok, init_rots (8, 3, 3), init_transes (8, 3)); the normals are not
        formed."""
        if cam_matrix_2 is not None and not np.array_equal(np.asarray(cam_matrix_1, np.float64), np.asarray(cam_matrix_2, np.float64)):
            raise PlpError(PLP_ERR_INVALID_ARG, "both frames have one camera matrix")
        d = model_homography_decompose(np.asarray(H_21, np.float64).reshape(3, 3), cam_matrix_1)
        return bool(d["ok"]), d["rots"], d["transes"]


class fundamental_solver(_perspective_solver):
    """Mirror of solve::fundamental_solver (solve/fundamental_solver.h)."""
    _S = "f"

    def get_best_F_21(self):
        return self._r["F_21"][0].copy()

    @staticmethod
    def decompose(F_21, cam_matrix_1, cam_matrix_2=None):
        """fundamental_solver::decompose (solve/fundamental_solver.cc:334-340; static, as in the reference): E_21 = (K^T * F_21) * K by D27 item e's
        products on the host, then essential_solver::decompose (the host build of D24 item c).  Returns (True, init_rots (4, 3, 3), init_transes (4, 3))."""
        from ._two_view import model_essential_decompose
        K = np.asarray(cam_matrix_1, np.float64).reshape(3, 3)
        if cam_matrix_2 is not None and not np.array_equal(K, np.asarray(cam_matrix_2, np.float64).reshape(3, 3)):
            raise PlpError(PLP_ERR_INVALID_ARG, "both frames have one camera matrix")
        mul = lambda A, B: np.array([[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)])
        d = model_essential_decompose(mul(mul(K.T, np.asarray(F_21, np.float64).reshape(3, 3)), K))
        return True, d["rots"], d["transes"]


# ---------------------------------------------------------------------------------------------------------------- from the chosen matrix to the pose
# the outputs of plp_perspective_pose_*: name -> (shape per problem given n_cap, dtype, optional)
PERSPECTIVE_POSE_OUTPUTS = dict(status=(lambda M: (), np.uint8, False), rot_ref_to_cur=(lambda M: (3, 3), np.float64, False),
                                trans_ref_to_cur=(lambda M: (3,), np.float64, False), hypothesis=(lambda M: (), np.int32, False),
                                num_valid=(lambda M: (8,), np.int32, False), parallax_deg=(lambda M: (8,), np.float32, False),
                                triangulated_pts=(lambda M: (M, 3), np.float64, False), is_triangulated=(lambda M: (M,), np.uint8, False),
                                hyp_is_triangulated=(lambda M: (8, M), np.uint8, True))


def perspective_pose_args(camera, fields, ptrs, img_bounds=None):
    """a plp_perspective_pose_args: the camera (a camera_model), its image bounds unless given, the scalar fields and the pointer fields"""
    a = _struct(perspective_pose_args_c, fields, ptrs)
    a.camera = camera_model_c.from_buffer_copy(camera)
    a.img_bounds[:] = [float(np.float32(v)) for v in (camera.img_bounds if img_bounds is None else img_bounds)]
    return a


def _perspective_pose_host(call, camera, choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated, parallax_deg_thr,
                           reproj_err_thr, counts_1, counts_2, img_bounds, outputs, out):
    """the numpy side of plp_perspective_pose_host and plp_model_perspective_pose_host: call(args struct) runs the entry"""
    ma = np.ascontiguousarray(match, np.int32)
    if ma.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "match must be (P, n_cap)")
    P_, M = ma.shape
    b1 = np.ascontiguousarray(bearing_1, np.float64).reshape(P_, M, 3)
    b2 = np.ascontiguousarray(bearing_2, np.float64)
    b2 = b2.reshape(P_, -1, 3) if P_ else b2.reshape(0, 0, 3)
    M2 = b2.shape[1]
    u1, u2 = _keypoints(undist_1).reshape(P_, M), _keypoints(undist_2).reshape(P_, M2)
    ch = np.ascontiguousarray(choice, np.uint8).reshape(P_)
    Hm, Fm = np.ascontiguousarray(H_21, np.float64).reshape(P_, 3, 3), np.ascontiguousarray(F_21, np.float64).reshape(P_, 3, 3)
    inl = np.ascontiguousarray(inliers, np.uint8).reshape(P_, M)
    c1, c2 = array_or_none(counts_1, np.int32, P_), array_or_none(counts_2, np.int32, P_)
    a = perspective_pose_args(camera, dict(P=P_, n_cap=M, m_cap=M2, min_num_triangulated=int(min_num_triangulated), parallax_deg_thr=float(parallax_deg_thr),
                                           reproj_err_thr=float(reproj_err_thr)),
                              host_ptrs(counts_1=c1, counts_2=c2, in_choice=ch, H_21=Hm, F_21=Fm, inliers=inl, match=ma, bearing_1=b1, bearing_2=b2, undist_1=u1,
                                        undist_2=u2), img_bounds)
    o = out_arrays(((k, (P_,) + shape(M), dt) for k, (shape, dt, optional) in PERSPECTIVE_POSE_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, PERSPECTIVE_POSE_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_perspective_pose(camera, choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated=50, parallax_deg_thr=1.0,
                           reproj_err_thr=4.0, counts_1=None, counts_2=None, img_bounds=None, outputs=None, out=None):
    """Host build of perspective::reconstruct_with_H / reconstruct_with_F (csrc/perspective_init.hpp, DESIGN.md section 5, D27 items e and h; no GPU
    needed): the arguments and the result of matcher.perspective_pose."""
    return _perspective_pose_host(model_call("plp_model_perspective_pose_host", "P"), camera, choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1,
                                  undist_2, min_num_triangulated, parallax_deg_thr, reproj_err_thr, counts_1, counts_2, img_bounds, outputs, out)


def model_homography_decompose(H_21, cam_matrix):
    """Host build of homography_solver::decompose (solve/homography_solver.cc:438-554; D27 item e; no GPU needed): H_21 (n, 3, 3) or (3, 3) under the
    camera matrix (3, 3) of both frames.  Returns dict(ok (n,) bool: false where the rank test fails, rots (n, 8, 3, 3), transes (n, 8, 3)) in the
    reference's order, without the leading axis for one matrix."""
    Hm = np.ascontiguousarray(H_21, np.float64)
    single = Hm.ndim == 2
    Hm = Hm.reshape(-1, 3, 3)
    K = np.ascontiguousarray(cam_matrix, np.float64).reshape(3, 3)
    n = len(Hm)
    ok, r, t = np.zeros(n, np.uint8), np.zeros((n, 8, 3, 3)), np.zeros((n, 8, 3))
    if lib().plp_model_homography_decompose_host(host_ptr(Hm), host_ptr(K), n, host_ptr(ok), host_ptr(r), host_ptr(t)) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_homography_decompose_host")
    o = dict(ok=ok.astype(bool), rots=r, transes=t)
    return {k: v[0] for k, v in o.items()} if single else o


class perspective_initializer:
    """Mirror of initialize::perspective (initialize/perspective.h, initialize/base.h): constructed on the reference frame (its camera, a camera_model
    of the perspective or fisheye model; undistorted key points; bearings) with the parameters of initialize::base; initialize(cur_undist_keypts,
    cur_bearings, ref_matches_with_cur) runs both RANSACs (the reference's own find_via_ransac for H and F), the choice and the reconstruction.
    mt: a matcher (the GPU entries), or None = the host builds.  samples_h / samples_f / seed: as matcher.perspective_ransac; given_H: (H_21,
    num_inliers) of the caller's graph-cut RANSAC, which then stands for the H RANSAC."""

    def __init__(self, camera, ref_undist_keypts, ref_bearings, num_ransac_iters=100, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, mt=None,
                 samples_h=None, samples_f=None, seed=0):
        self._cam = camera
        self._u1 = _keypoints(ref_undist_keypts).reshape(1, -1)
        self._b1 = np.ascontiguousarray(ref_bearings, np.float64).reshape(1, -1, 3)
        self._iters = int(num_ransac_iters)
        self._kw = dict(min_num_triangulated=min_num_triangulated, parallax_deg_thr=parallax_deg_thr, reproj_err_thr=reproj_err_thr)
        self._mt, self._samples, self._seed = mt, dict(samples_h=samples_h, samples_f=samples_f), seed
        self.ransac, self._r = None, None

    def initialize(self, cur_undist_keypts, cur_bearings, ref_matches_with_cur, given_H=None):
        u2 = _keypoints(cur_undist_keypts).reshape(1, -1)
        b2 = np.ascontiguousarray(cur_bearings, np.float64).reshape(1, -1, 3)
        match = np.ascontiguousarray(ref_matches_with_cur, np.int32).reshape(1, -1)
        ransac = model_perspective_ransac if self._mt is None else self._mt.perspective_ransac
        pose = model_perspective_pose if self._mt is None else self._mt.perspective_pose
        g = {} if given_H is None else dict(given_H_21=np.asarray(given_H[0], np.float64).reshape(1, 9), given_H_num_inliers=[int(given_H[1])])
        self.ransac = e = ransac(self._u1, u2, match, iters=self._iters, recompute=True, seed=self._seed, **self._samples, **g)
        self._r = pose(self._cam, e["choice"], e["H_21"], e["F_21"], e["inliers"], match, self._b1, b2, self._u1, u2, **self._kw)
        return int(self._r["status"][0]) == 0

    def get_rotation_ref_to_cur(self):
        return self._r["rot_ref_to_cur"][0].copy()

    def get_translation_ref_to_cur(self):
        return self._r["trans_ref_to_cur"][0].copy()

    def get_triangulated_pts(self):
        return self._r["triangulated_pts"][0].copy()

    def get_triangulated_flags(self):
        return self._r["is_triangulated"][0].astype(bool)
