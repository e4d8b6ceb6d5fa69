"""Map initialisation, from the essential matrix to the pose: bearing_vector::reconstruct_with_E (include/plp_front.h: plp_two_view_pose_*, the
plp_model_* host builds; DESIGN.md section 5, D24 items c, f, g): the numpy side of the host-pointer entry and the host builds, and the mirror
class of initialize::bearing_vector."""

import ctypes as C

import numpy as np

from ._abi import ESSENTIAL_OK, KP_DTYPE, TWO_VIEW_NO_SOLUTION, TWO_VIEW_OK, _struct, camera_model_c, two_view_pose_args_c
from ._core import PLP_ERR_INVALID_ARG, PlpError, lib
from ._essential import model_essential_ransac
from ._marshal import array_or_none, host_ptr, host_ptrs, model_call, out_arrays, set_outputs, wanted

# the outputs of plp_two_view_pose_*: name -> (shape per problem given n_cap, dtype, optional)
TWO_VIEW_OUTPUTS = dict(status=(lambda M: (), np.uint8, False), rot_ref_to_cur=(lambda M: (3, 3), np.float64, False),
                        trans_ref_to_cur=(lambda M: (3,), np.float64, False), hypothesis=(lambda M: (), np.int32, False),
                        num_valid=(lambda M: (4,), np.int32, False), parallax_deg=(lambda M: (4,), np.float32, False),
                        triangulated_pts=(lambda M: (M, 3), np.float64, False), is_triangulated=(lambda M: (M,), np.uint8, False),
                        hyp_is_triangulated=(lambda M: (4, M), np.uint8, True))


def two_view_args(camera, fields, ptrs, img_bounds=None):
    """a plp_two_view_pose_args: the camera (a camera_model), its image bounds unless given, the scalar fields and the pointer fields"""
    a = _struct(two_view_pose_args_c, fields, ptrs)
    a.camera = camera_model_c.from_buffer_copy(camera)
    a.img_bounds[:] = [float(np.float32(v)) for v in (camera.img_bounds if img_bounds is None else img_bounds)]
    return a


def _two_view_inputs(camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated, parallax_deg_thr, reproj_err_thr,
                     depth_is_positive, in_status, counts_1, counts_2, img_bounds):
    ma = np.ascontiguousarray(match, np.int32)
    if ma.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "match must be (P, n_cap)")
    P_, M = ma.shape
    b1 = np.ascontiguousarray(bearing_1, np.float64).reshape(P_, M, 3)
    b2 = np.ascontiguousarray(bearing_2, np.float64)
    b2 = b2.reshape(P_, -1, 3) if P_ else b2.reshape(0, 0, 3)
    M2 = b2.shape[1]
    u1, u2 = np.ascontiguousarray(undist_1, KP_DTYPE).reshape(P_, M), np.ascontiguousarray(undist_2, KP_DTYPE).reshape(P_, M2)
    E = np.ascontiguousarray(E_21, np.float64).reshape(P_, 3, 3)
    inl = np.ascontiguousarray(inliers, np.uint8).reshape(P_, M)
    st, c1, c2 = array_or_none(in_status, np.uint8, P_), array_or_none(counts_1, np.int32, P_), array_or_none(counts_2, np.int32, P_)
    a = two_view_args(camera, dict(P=P_, n_cap=M, m_cap=M2, min_num_triangulated=int(min_num_triangulated), parallax_deg_thr=float(parallax_deg_thr),
                                   reproj_err_thr=float(reproj_err_thr), depth_is_positive=int(bool(depth_is_positive))),
                      host_ptrs(counts_1=c1, counts_2=c2, in_status=st, E_21=E, inliers=inl, match=ma, bearing_1=b1, bearing_2=b2, undist_1=u1, undist_2=u2), img_bounds)
    return a, (ma, b1, b2, u1, u2, E, inl, st, c1, c2), P_, M


def _two_view_pose_host(call, camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated, parallax_deg_thr, reproj_err_thr,
                        depth_is_positive, in_status, counts_1, counts_2, img_bounds, outputs, out):
    """the numpy side of plp_two_view_pose_host and plp_model_two_view_pose_host: call(args struct) runs the entry"""
    a, keep, P_, M = _two_view_inputs(camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated, parallax_deg_thr,
                                      reproj_err_thr, depth_is_positive, in_status, counts_1, counts_2, img_bounds)
    o = out_arrays(((k, (P_,) + shape(M), dt) for k, (shape, dt, optional) in TWO_VIEW_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, TWO_VIEW_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_two_view_pose(camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated=50, parallax_deg_thr=1.0,
                        reproj_err_thr=4.0, depth_is_positive=False, in_status=None, counts_1=None, counts_2=None, img_bounds=None, outputs=None, out=None):
    """Host build of bearing_vector::reconstruct_with_E (csrc/two_view.hpp; no GPU needed): the arguments and the result
    of matcher.two_view_pose."""
    return _two_view_pose_host(model_call("plp_model_two_view_pose_host", "P"), camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2,
                               min_num_triangulated, parallax_deg_thr, reproj_err_thr, depth_is_positive, in_status, counts_1, counts_2, img_bounds, outputs, out)


def model_essential_decompose(E_21):
    """Host build of essential_solver::decompose (solve/essential_solver.cc:156-186; D24 item c; no GPU needed): E_21 (n, 3, 3) or (3, 3).  Returns
    dict(rots (n, 4, 3, 3), transes (n, 4, 3)): the four hypotheses in the reference's order, without the leading axis for one matrix."""
    E = np.ascontiguousarray(E_21, np.float64)
    single = E.ndim == 2
    E = E.reshape(-1, 3, 3)
    n = len(E)
    r, t = np.zeros((n, 2, 3, 3)), np.zeros((n, 3))
    if lib().plp_model_essential_decompose_host(host_ptr(E), n, host_ptr(r), host_ptr(t)) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_essential_decompose_host")
    o = dict(rots=np.stack([r[:, 0], r[:, 0], r[:, 1], r[:, 1]], 1), transes=np.stack([t, -t, t, -t], 1))
    return {k: v[0] for k, v in o.items()} if single else o


def model_check_pose(camera, rot, trans, inliers, match, bearing_1, bearing_2, undist_1, undist_2, reproj_err_thr=4.0, depth_is_positive=False, count_2=None,
                     img_bounds=None):
    """Host build of initialize::base::check_pose (initialize/base.cc:123-243; D24 item f; no GPU needed) of one (rot, trans) against one problem
    given without the leading axis.  Returns dict(num_valid, parallax_deg (f32), pts (n_cap, 3), is_triangulated (n_cap,), code (n_cap,): 0 = no
    inlier match, 1 .. 7 the `continue` the match takes, 8 valid with a small parallax, 9 valid and triangulated)."""
    ma = np.ascontiguousarray(match, np.int32).reshape(1, -1)
    M = ma.shape[1]
    c2 = None if count_2 is None else np.array([count_2], np.int32)
    a, keep, _, _ = _two_view_inputs(camera, np.zeros((1, 3, 3)), np.asarray(inliers).reshape(1, M), ma, np.asarray(bearing_1).reshape(1, M, 3),
                                     np.asarray(bearing_2).reshape(1, -1, 3), np.asarray(undist_1).reshape(1, M), np.asarray(undist_2).reshape(1, -1), 50, 1.0,
                                     reproj_err_thr, depth_is_positive, None, None, c2, img_bounds)
    R, t = np.ascontiguousarray(rot, np.float64).reshape(3, 3), np.ascontiguousarray(trans, np.float64).reshape(3)
    nv, pd = np.zeros(1, np.int32), np.zeros(1, np.float32)
    o = dict(pts=np.zeros((M, 3)), is_triangulated=np.zeros(M, np.uint8), code=np.zeros(M, np.uint8))
    if lib().plp_model_check_pose_host(C.byref(a), host_ptr(R), host_ptr(t), host_ptr(nv), host_ptr(pd), host_ptr(o["pts"], False),
                                       host_ptr(o["is_triangulated"], False), host_ptr(o["code"], False)) != 1:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_check_pose_host")
    return dict(o, num_valid=int(nv[0]), parallax_deg=np.float32(pd[0]))


class bearing_vector_initializer:
    """Mirror of initialize::bearing_vector (initialize/bearing_vector.h, initialize/base.h): constructed on the reference frame (its camera, a
    camera_model; undistorted key points, KP_DTYPE; bearings) with the parameters of initialize::base; initialize(cur_undist_keypts, cur_bearings,
    ref_matches_with_cur) runs the eight-point RANSAC and the reconstruction.  mt: a matcher (the GPU entries), or None = the host builds.
    samples / seed: as matcher.essential_ransac."""

    def __init__(self, camera, ref_undist_keypts, ref_bearings, num_ransac_iters=100, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, mt=None,
                 samples=None, seed=0):
        self._cam = camera
        self._u1 = np.ascontiguousarray(ref_undist_keypts, KP_DTYPE).reshape(1, -1)
        self._b1 = np.ascontiguousarray(ref_bearings, np.float64).reshape(1, -1, 3)
        self._iters = int(num_ransac_iters)
        self._kw = dict(min_num_triangulated=min_num_triangulated, parallax_deg_thr=parallax_deg_thr, reproj_err_thr=reproj_err_thr)
        self._mt, self._samples, self._seed = mt, samples, seed
        self.essential, self._r = None, None

    def initialize(self, cur_undist_keypts, cur_bearings, ref_matches_with_cur):
        u2 = np.ascontiguousarray(cur_undist_keypts, KP_DTYPE).reshape(1, -1)
        b2 = np.ascontiguousarray(cur_bearings, np.float64).reshape(1, -1, 3)
        match = np.ascontiguousarray(ref_matches_with_cur, np.int32).reshape(1, -1)
        ransac = model_essential_ransac if self._mt is None else self._mt.essential_ransac
        pose = model_two_view_pose if self._mt is None else self._mt.two_view_pose
        self.essential = e = ransac(self._b1, b2, match, iters=self._iters, recompute=True, samples=self._samples, seed=self._seed)
        self._r = pose(self._cam, e["E_21"], e["inliers"], match, self._b1, b2, self._u1, u2, in_status=e["status"], **self._kw)   # bearing_vector.cc:72-81
        return int(e["status"][0]) == ESSENTIAL_OK and int(self._r["status"][0]) == TWO_VIEW_OK

    def get_rotation_ref_to_cur(self):
        return self._r["rot_ref_to_cur"][0].copy()

    def get_translation_ref_to_cur(self):
        return self._r["trans_ref_to_cur"][0].copy()

    def get_triangulated_pts(self):
        return self._r["triangulated_pts"][0].copy()

    def get_triangulated_flags(self):
        return self._r["is_triangulated"][0].astype(bool)
