"""structure-plp-slam_amd — MI355X-native feature front-end and matcher for Structure-PLP-SLAM.

The product is ``libplp_front.so`` (hand-written HIP kernels for gfx950 behind the C ABI declared
in ``include/plp_front.h``).  This package is the thin Python host mirror used by the tests and
the bench: class and method names follow the reference's C++ interface
(``feature::orb_extractor`` — src/PLPSLAM/feature/orb_extractor.h:38-176).  There is no CPU
fallback: if the shared library is missing or no GPU is visible the calls raise.

Three modules carry what every mirror shares: ``_core`` (the library handle and its symbol table), ``_abi`` (the struct mirrors and
constants of the header) and ``_marshal`` (arrays, tensors and streams to the ABI's arguments).  Their names are re-exported here.
The mirrors below are still one file; each subsystem is to move to a module of its own over those three, a pure move per change that
``tests/golden/package_surface.txt`` guards (everything stays an attribute of the package), with ``matcher`` importing the subsystems.
"""
import ctypes as C
import math
import os
import pathlib
import subprocess

import numpy as np

# _lib below is the value at import time (None), kept as a name of the package only: the loaded handle is _core._lib, read through lib()
from ._core import (LIB_PATH, PLP_ERR_CAPACITY, PLP_ERR_HIP, PLP_ERR_INVALID_ARG, PLP_ERR_NO_DEVICE, PLP_ERR_OVERFLOW, PLP_ERR_UNSUPPORTED, PLP_OK, PlpError,
                    ROOT, _API, _I32, _PKG, _SZ, _VP, _check, _lib, _p, api_symbols, build, lib)
from ._abi import *        # noqa: F401,F403  every struct mirror, record dtype, enum and limit of include/plp_front.h
from ._abi import _struct
from ._global_ba import (GLOBAL_BA_OUTPUTS, LOOP_BA_PROPAGATE_OUTPUTS, _chol_dense, _global_ba_host, _global_ba_kw, _loop_ba_propagate_host, global_bundle_adjuster,
                         loop_bundle_adjuster, model_chol_dense, model_global_ba, model_loop_ba_propagate)
from ._essential import (ESSENTIAL_OUTPUTS, _essential_ransac_host, essential_solver, model_essential_check, model_essential_draw, model_essential_fit,
                         model_essential_ransac)
from ._two_view import (TWO_VIEW_OUTPUTS, _two_view_pose_host, bearing_vector_initializer, model_check_pose, model_essential_decompose, model_two_view_pose,
                        two_view_args)
from ._perspective import (PERSPECTIVE_POSE_OUTPUTS, PERSPECTIVE_RANSAC_OUTPUTS, _perspective_pose_host, _perspective_ransac_host, fundamental_solver,
                           homography_solver, model_fundamental_check, model_fundamental_fit, model_homography_check, model_homography_decompose,
                           model_homography_fit, model_normalize_keypoints, model_perspective_draw, model_perspective_pose, model_perspective_ransac,
                           perspective_initializer, perspective_pose_args)
from ._line_update import (CORRECT_LINE_ERASED, CORRECT_LINE_NO_REF, CORRECT_LINE_NO_VERTEX, CORRECT_LINE_OK, LINE_MOVE_OUTPUTS, TRIM_DEPTH_POSITIVE, TRIM_INDEX_RANGE,
                           TRIM_MAX_CHANGE, TRIM_MAX_CHANGE_THR, TRIM_NO_REF, TRIM_NOT_OBSERVED, TRIM_OK, TRIM_OUTPUTS, TRIM_REJECTED, TRIM_SKIPPED,
                           correct_landmark_lines_args_c, line_update_entries, loop_ba_propagate_lines_args_c, model_correct_landmark_lines,
                           model_loop_ba_propagate_lines, model_trim_line_endpoints, trim_line_endpoints_args_c)
from ._marshal import _rows_u8, array_or_none, dev_ptr, dev_ptrs, host_ptr, host_ptrs, model_call, model_draw, out_arrays, set_outputs, stream_handle, wanted


def model_quadtree(xys, level_w, level_h, quota):
    """Host model of the quadtree kernel (no GPU needed).  xys: (n,3) int32 (x, y, score)."""
    xys = np.ascontiguousarray(xys, np.int32).reshape(-1, 3)
    out = np.zeros(max(len(xys), 1), np.int32)
    m = lib().plp_model_quadtree_host(_p(xys), len(xys), level_w, level_h, quota, _p(out))
    return out[:m].copy()


def model_quadtree_rank_sort(keys, shift=0):
    """Host model of the quadtree kernel's rank sort of small levels (no GPU needed): the indices of `keys` in the order of a stable sort by keys >> shift"""
    k = np.ascontiguousarray(keys, np.uint32)
    perm = np.zeros(max(len(k), 1), np.uint32)
    assert lib().plp_model_quadtree_rank_sort_host(_p(k), len(k), int(shift), _p(perm)) == len(k)
    return perm[:len(k)].copy()


def model_seed_introsort(entries, depth_limit=-1, skip_key=0):
    """Host model of the exact seed sort: std::__introsort_loop on entries keyed by bits 20..29 (larger first), as rank-paired partitions; parts
    that can only hold keys below skip_key are left alone (include/plp_front.h); no GPU"""
    e = np.ascontiguousarray(entries, np.uint32).copy()
    assert lib().plp_model_seed_introsort_host(_p(e), e.size, int(depth_limit), int(skip_key)) == 0
    return e


def seed_introsort_debug(entries, depth_limit=-1, skip_key=0, variant=0, device=0, return_live=False):
    """The KERNEL's introsort loop on caller-made entries (one workgroup), with a chosen recursion budget and skip key; variant 0 / 1: the kernel
    configuration of large / small batches.  return_live: also the length of the live part (entries behind it are unspecified: plp_front.h)"""
    e = np.ascontiguousarray(entries, np.uint32).copy()
    nl = C.c_int32(e.size)
    _check(lib().plp_seed_introsort_debug(int(device), _p(e), e.size, int(depth_limit), int(skip_key), int(variant), C.byref(nl)))
    return (e, nl.value) if return_live else e


def seed_sort_tile_ranks(n_frame, n_segment=None, variant=0, return_masks=False):
    """How the exact seed sort's kernel (variant 0 / 1 as in seed_introsort_debug) partitions a segment of n_segment entries of a frame of n_frame: the ranks per
    side of the LDS tile its stoppers' entries change sides through.  return_masks: also whether the chunk masks are in LDS.  No GPU"""
    lm = C.c_int32(0)
    r = lib().plp_seed_sort_tile_ranks(int(n_frame), int(n_frame if n_segment is None else n_segment), int(variant), C.byref(lm))
    if r < 0:
        raise ValueError("bad arguments")
    return (r, bool(lm.value)) if return_masks else r


def model_index_sort(sizes, depth_limit=-1):
    """Host model of the matchers' bin ranking (libstdc++ std::sort order of the indices by size, descending); no GPU needed"""
    sz = np.ascontiguousarray(sizes, np.int32)
    idx = np.zeros(len(sz), np.uint32)
    assert lib().plp_model_index_sort_host(_p(sz), len(sz), int(depth_limit), _p(idx)) == len(sz)
    return idx


def model_sincos(a):
    """Host model of the LSD gradient kernel's cos / sin fast path (no GPU needed): (cos f32, sin f32, proven bool)"""
    a = np.ascontiguousarray(a, np.float32)
    c = np.zeros(a.shape, np.float32); s = np.zeros(a.shape, np.float32); ok = np.zeros(a.shape, np.uint8)
    lib().plp_model_sincos_host(_p(a), a.size, _p(c), _p(s), _p(ok))
    return c, s, ok.astype(bool)


def _landmark_geometry_host(call, lines, pose, feats, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, scale_factors, scale_factors_lsd, skip, counts,
                            out):
    """the numpy side of plp_landmark[_line]_geometry_host and plp_model_landmark_geometry_host: call(args struct) runs the entry"""
    po = np.ascontiguousarray(pose, np.float64).reshape(-1, 15)
    F = len(po)
    ft = np.ascontiguousarray(feats, KL_DTYPE if lines else KP_DTYPE).reshape(F, -1)
    M = ft.shape[1]
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 6 if lines else 3)
    L = len(pw)
    rk = np.ascontiguousarray(ref_kf, np.int32).reshape(L)
    oo = np.ascontiguousarray(obs_offsets, np.int32).reshape(L + 1)
    ok = np.ascontiguousarray(obs_kf, np.int32).reshape(-1)
    oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
    if len(ok) != len(oi) or (L and int(oo[L]) > len(ok)):
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_kf and obs_idx must hold obs_offsets[L] entries each")
    if L and len(ok) == 0:
        ok, oi = np.zeros(1, np.int32), np.zeros(1, np.int32)            # lists without an entry: the arrays are still required
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(L)
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    sl = np.ascontiguousarray(scale_factors_lsd, np.float32).reshape(-1) if lines else None
    o = out_arrays((("min_dist", (L,), np.float32), ("max_dist", (L,), np.float32), ("status", (L,), np.uint8))
                   + (() if lines else (("normal", (L, 3), np.float64),)), out)
    a = _struct(landmark_geometry_args_c, dict(F=F, cap=M, L=L, num_levels=len(sf), num_levels_lsd=len(sl) if lines else 0), host_ptrs(
        pose=po, counts=cn, keypts=None if lines else ft, keylines=ft if lines else None, scale_factors=sf, scale_factors_lsd=sl, pos_w=pw, ref_kf=rk,
        skip=sk, obs_offsets=oo, obs_kf=ok, obs_idx=oi, out_mean_normal=o.get("normal"), out_min_valid_dist=o["min_dist"], out_max_valid_dist=o["max_dist"],
        out_status=o["status"]))
    call(a)
    return o


def model_landmark_geometry(pose, feats, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, scale_factors, scale_factors_lsd=None, skip=None, counts=None,
                            lines=False, out=None):
    """Host build of landmark::update_normal_and_depth / Line::update_information (csrc/landmark_geometry.hpp; no GPU
    needed): the arguments and the result of matcher.landmark_geometry (lines: matcher.landmark_line_geometry)."""
    return _landmark_geometry_host(model_call("plp_model_landmark_geometry_host", "L", int(bool(lines))), bool(lines), pose, feats, pos_w, ref_kf, obs_offsets,
                                   obs_kf, obs_idx, scale_factors, scale_factors_lsd, skip, counts, out)


def model_bow_score(wa, va, wb, vb):
    """Host build of the BowVector score (csrc/bow_score.hpp; no GPU needed): DBoW2's L1Scoring::score of two vectors
    given as ascending word ids and values, as f64 before the narrowing to float.  Restated from the published algorithm, parity unpinned."""
    wa = np.ascontiguousarray(wa, np.uint32).reshape(-1); va = np.ascontiguousarray(va, np.float64).reshape(-1)
    wb = np.ascontiguousarray(wb, np.uint32).reshape(-1); vb = np.ascontiguousarray(vb, np.float64).reshape(-1)
    if len(wa) != len(va) or len(wb) != len(vb):
        raise PlpError(PLP_ERR_INVALID_ARG, "words and values must have the same length")
    return float(lib().plp_model_bow_score_host(host_ptr(wa), host_ptr(va), len(wa), host_ptr(wb), host_ptr(vb), len(wb)))


def model_null_vector4(A):
    """Host build of the null vector of the point triangulation (csrc/null4.hpp; no GPU needed).  A: (n, 4, 4) or
    (4, 4) f64.  Returns (v (n, 4) f64, sweeps (n,) i32): the column of V with the smallest |A v|, and the sweeps that rotated (30 = limit)."""
    A = np.ascontiguousarray(A, np.float64)
    single = A.ndim == 2
    A = A.reshape(-1, 16)
    v = np.zeros((len(A), 4), np.float64); sw = np.zeros(len(A), np.int32)
    assert lib().plp_model_null_vector4_host(_p(A), len(A), _p(v), _p(sw)) == len(A)
    return (v[0], int(sw[0])) if single else (v, sw)


def model_sym_eig4_max(N):
    """Host build of the eigenvector Horn's method needs (csrc/sim3.hpp; no GPU needed).  N: (n, 4, 4) or (4, 4) f64,
    symmetric (the upper triangle is read).  Returns (v (n, 4) f64, sweeps (n,) i32): the unit eigenvector of the largest eigenvalue (ties: the
    lowest column; sign unspecified) and the sweeps that rotated (30 = limit)."""
    N = np.ascontiguousarray(N, np.float64)
    single = N.ndim == 2
    N = N.reshape(-1, 16)
    v = np.zeros((len(N), 4), np.float64); sw = np.zeros(len(N), np.int32)
    assert lib().plp_model_sym_eig4_max_host(host_ptr(N), len(N), host_ptr(v), host_ptr(sw)) == len(N)
    return (v[0], int(sw[0])) if single else (v, sw)


def model_horn_sim3(pts_1, pts_2, fix_scale=False):
    """Host build of sim3_solver::compute_Sim3 (solve/sim3_solver.cc:193-288; csrc/sim3.hpp, D13; no GPU needed).  pts_1 / pts_2: (n, 3, 3) or
    (3, 3) f64, column c = sample c.  Returns dict(rot_12, rot_21 (n, 3, 3) f64, trans_12, trans_21 (n, 3) f64, scale_12, scale_21 (n,) f32,
    sweeps (n,) i32); without the leading axis for a single pair."""
    a = np.ascontiguousarray(pts_1, np.float64); b = np.ascontiguousarray(pts_2, np.float64)
    single = a.ndim == 2
    a = a.reshape(-1, 9); b = b.reshape(-1, 9)
    if len(a) != len(b):
        raise PlpError(PLP_ERR_INVALID_ARG, "pts_1 and pts_2 must hold the same number of 3 x 3 matrices")
    n = len(a)
    o = dict(rot_12=np.zeros((n, 3, 3)), trans_12=np.zeros((n, 3)), scale_12=np.zeros(n, np.float32), rot_21=np.zeros((n, 3, 3)), trans_21=np.zeros((n, 3)),
             scale_21=np.zeros(n, np.float32), sweeps=np.zeros(n, np.int32))
    assert lib().plp_model_horn_sim3_host(host_ptr(a), host_ptr(b), n, int(bool(fix_scale)), host_ptr(o["rot_12"]), host_ptr(o["trans_12"]),
                                          host_ptr(o["scale_12"]), host_ptr(o["rot_21"]), host_ptr(o["trans_21"]), host_ptr(o["scale_21"]), host_ptr(o["sweeps"])) == n
    return {k: v[0] for k, v in o.items()} if single else o


def model_sim3_draw(seed, p, iters, num_common, iter0=0):
    """The samples plp_sim3_ransac_* draw for problem p when the caller passes none (D13's generator; no GPU needed): (iters, 3) i32"""
    return model_draw("plp_model_sim3_draw_host", "num_common must be at least 3, iters non-negative", seed, p, iters, iter0, 3, num_common)
# the outputs of plp_sim3_ransac_*: name -> (shape per problem given (n_cap, iters), dtype, optional)
SIM3_OUTPUTS = dict(status=(lambda M, I: (), np.uint8, False), num_common=(lambda M, I: (), np.int32, False), rot_12=(lambda M, I: (3, 3), np.float64, False),
                    trans_12=(lambda M, I: (3,), np.float64, False), scale_12=(lambda M, I: (), np.float32, False),
                    num_inliers=(lambda M, I: (), np.int32, False), best_iter=(lambda M, I: (), np.int32, False),
                    inliers=(lambda M, I: (M,), np.uint8, True), hyp_inliers=(lambda M, I: (I,), np.int32, True))


def _sim3_ransac_host(call, camera, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, level_sigma_sq_1, level_sigma_sq_2, iters, fix_scale,
                      min_num_inliers, samples, seed, counts, outputs, out):
    """the numpy side of plp_sim3_ransac_host and plp_model_sim3_ransac_host: call(args struct) runs the entry"""
    va = np.ascontiguousarray(valid, np.uint8)
    if va.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "valid must be (P, n_cap)")
    P_, M = va.shape
    w1 = np.ascontiguousarray(pos_w_1, np.float64).reshape(P_, M, 3); w2 = np.ascontiguousarray(pos_w_2, np.float64).reshape(P_, M, 3)
    o1 = np.ascontiguousarray(octave_1, np.int32).reshape(P_, M); o2 = np.ascontiguousarray(octave_2, np.int32).reshape(P_, M)
    p1 = np.ascontiguousarray(pose_1, np.float64).reshape(P_, 15); p2 = np.ascontiguousarray(pose_2, np.float64).reshape(P_, 15)
    s1 = np.ascontiguousarray(level_sigma_sq_1, np.float32).reshape(-1); s2 = np.ascontiguousarray(level_sigma_sq_2, np.float32).reshape(-1)
    if len(s1) != len(s2):
        raise PlpError(PLP_ERR_INVALID_ARG, "level_sigma_sq_1 and level_sigma_sq_2 must have the same length")
    I = int(iters)
    sm = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(P_, I, 3)
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(P_)
    o = out_arrays(((k, (P_,) + shape(M, max(I, 0)), dt) for k, (shape, dt, optional) in SIM3_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    a = _struct(sim3_ransac_args_c, dict(P=P_, n_cap=M, fix_scale=int(bool(fix_scale)), min_num_inliers=int(min_num_inliers), iters=I,
                                         seed=int(seed) & 0xFFFFFFFFFFFFFFFF, num_levels=len(s1)), host_ptrs(
        level_sigma_sq_1=s1, level_sigma_sq_2=s2, counts=cn, valid=va, pos_w_1=w1, pos_w_2=w2, octave_1=o1, octave_2=o2, pose_1=p1, pose_2=p2, samples=sm))
    set_outputs(a, SIM3_OUTPUTS, o, host_ptr)
    a.camera = camera_model_c.from_buffer_copy(camera)
    call(a)
    return o


def model_sim3_ransac(camera, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, level_sigma_sq_1, level_sigma_sq_2, iters=200, fix_scale=False,
                      min_num_inliers=20, samples=None, seed=0, counts=None, outputs=None, out=None):
    """Host build of solve::sim3_solver's constructor and find_via_ransac (csrc/sim3.hpp; no GPU needed): the arguments
    and the result of matcher.sim3_ransac."""
    return _sim3_ransac_host(model_call("plp_model_sim3_ransac_host", "P"), camera, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2,
                             level_sigma_sq_1, level_sigma_sq_2, iters, fix_scale, min_num_inliers, samples, seed, counts, outputs, out)


class sim3_solver:
    """Mirror of solve::sim3_solver (solve/sim3_solver.h) over the flattened lists of its constructor's loop (include/plp_front.h,
    plp_sim3_ransac_args): valid / pos_w_1 / pos_w_2 / octave_1 / octave_2 per key point of key frame 1, the two pose rows and sigma tables.
    mt: a matcher (the GPU entry), or None = the host build.  samples / seed: as matcher.sim3_ransac."""

    def __init__(self, camera, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, level_sigma_sq_1, level_sigma_sq_2, fix_scale=False,
                 min_num_inliers=20, mt=None, samples=None, seed=0):
        n = len(np.asarray(valid).reshape(-1))
        self._in = (camera, np.asarray(valid).reshape(1, n), np.asarray(pos_w_1).reshape(1, n, 3), np.asarray(pos_w_2).reshape(1, n, 3),
                    np.asarray(octave_1).reshape(1, n), np.asarray(octave_2).reshape(1, n), np.asarray(pose_1).reshape(1, 15), np.asarray(pose_2).reshape(1, 15),
                    level_sigma_sq_1, level_sigma_sq_2)
        self._kw = dict(fix_scale=fix_scale, min_num_inliers=min_num_inliers, samples=samples, seed=seed)
        self._mt = mt
        self._r = None

    def find_via_ransac(self, max_num_iter):
        fn = model_sim3_ransac if self._mt is None else self._mt.sim3_ransac
        self._r = fn(*self._in, iters=int(max_num_iter), **self._kw)

    def solution_is_valid(self):
        return self._r is not None and int(self._r["status"][0]) == SIM3_OK

    def get_best_rotation_12(self):
        return self._r["rot_12"][0].copy()

    def get_best_translation_12(self):
        return self._r["trans_12"][0].copy()

    def get_best_scale_12(self):
        return float(self._r["scale_12"][0])

    def get_inliers(self):
        """the inlier flags of the best hypothesis per key point of key frame 1 (not in the reference's surface: count_inliers' vector)"""
        return self._r["inliers"][0].astype(bool)


# the outputs of plp_plane_ransac_*: name -> (shape per problem given (n_cap, iters), dtype, optional)
PLANE_RANSAC_OUTPUTS = dict(status=(lambda M, I: (), np.uint8, False), flags=(lambda M, I: (), np.uint8, False),
                            equation=(lambda M, I: (4,), np.float64, False), best_error=(lambda M, I: (), np.float64, False),
                            best_iter=(lambda M, I: (), np.int32, False), last_iter=(lambda M, I: (), np.int32, False),
                            num_inliers=(lambda M, I: (), np.int32, False), inliers=(lambda M, I: (M,), np.uint8, False),
                            hyp_residual=(lambda M, I: (I,), np.float64, True), hyp_inliers=(lambda M, I: (I,), np.int32, True),
                            hyp_error=(lambda M, I: (I,), np.float64, True))


def plane_sample_size(mode, n, points_per_ransac):
    """the samples of one hypothesis: POINTS_PER_RANSAC (CREATE), the smallest m with !(m < n * 0.8) (UPDATE, planar_mapping_module.cc:620)"""
    if int(mode) == PLANE_CREATE:
        return int(points_per_ransac)
    m = int(float(n) * 0.8)
    while float(m) < float(n) * 0.8:
        m += 1
    return m


def _plane_ransac_host(call, mode, pos_w, flags, dist_thresh, error_thresh, points_per_ransac, min_points_before_ransac, iters, inliers_ratio_thr,
                       best_error_in, equation_in, samples, seed, counts, outputs, out):
    """the numpy side of plp_plane_ransac_host and plp_model_plane_ransac_host: call(args struct) runs the entry"""
    fl = np.ascontiguousarray(flags, np.uint8)
    if fl.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "flags must be (P, n_cap)")
    P_, M = fl.shape
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(P_, M, 3)
    vec = lambda v, w=(): None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (P_,) + w))
    dt_, et_, be, eq = vec(dist_thresh), vec(error_thresh), vec(best_error_in), vec(equation_in, (4,))
    I = int(iters)
    sm = None if samples is None else np.ascontiguousarray(samples, np.int32)
    if sm is not None and (sm.ndim != 3 or sm.shape[:2] != (P_, I)):
        raise PlpError(PLP_ERR_INVALID_ARG, "samples must be (P, iters, m_cap)")
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(P_)
    o = out_arrays(((k, (P_,) + shape(M, max(I, 0)), dt) for k, (shape, dt, optional) in PLANE_RANSAC_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    a = _struct(plane_ransac_args_c, dict(mode=int(mode), P=P_, n_cap=M, points_per_ransac=int(points_per_ransac),
                                          min_points_before_ransac=int(min_points_before_ransac), iters=I, inliers_ratio_thr=float(inliers_ratio_thr),
                                          seed=int(seed) & 0xFFFFFFFFFFFFFFFF, m_cap=0 if sm is None else sm.shape[2]), host_ptrs(
        counts=cn, pos_w=pw, flags=fl, dist_thresh=dt_, error_thresh=et_, best_error_in=be, equation_in=eq, samples=sm))
    set_outputs(a, PLANE_RANSAC_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_plane_ransac(mode, pos_w, flags, dist_thresh, error_thresh, points_per_ransac=18, min_points_before_ransac=12, iters=50, inliers_ratio_thr=0.7,
                       best_error_in=None, equation_in=None, samples=None, seed=0, counts=None, outputs=None, out=None):
    """Host build of Planar_Mapping_module's RANSAC (csrc/plane_fit.hpp; no GPU needed): the arguments and the result
    of matcher.plane_ransac."""
    return _plane_ransac_host(model_call("plp_model_plane_ransac_host", "P"), mode, pos_w, flags, dist_thresh, error_thresh, points_per_ransac,
                              min_points_before_ransac, iters, inliers_ratio_thr, best_error_in, equation_in, samples, seed, counts, outputs, out)


def model_plane_fit(pos_w, lists):
    """Host build of estimate_plane_SVD (planar_mapping_module.cc:735-771 as D19 item 3 writes it down; no GPU needed).  pos_w: (n_points, 3) f64,
    lists: index lists into it.  Returns (equation (n, 4), residual (n,), sweeps (n,) i32: the Jacobi sweeps that rotated)."""
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    lists = [np.asarray(l, np.int32).reshape(-1) for l in lists]
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), np.int32)
    n = len(lists)
    eq = np.zeros((n, 4)); res = np.zeros(n); sw = np.zeros(n, np.int32)
    if lib().plp_model_plane_fit_host(host_ptr(pw), len(pw), host_ptr(idx), host_ptr(off), n, host_ptr(eq), host_ptr(res), host_ptr(sw)) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_plane_fit_host")
    return eq, res, sw


def model_plane_draw(seed, p, iters, m, n_eligible, iter0=0):
    """The ranks plp_plane_ransac_* draw for problem p when the caller passes none (D19 item 2; no GPU needed): (iters, m) i32"""
    return model_draw("plp_model_plane_draw_host", "plp_model_plane_draw_host: n_eligible must be at least 1", seed, p, iters, iter0, m, m, n_eligible)


def _plane_refine_host(call, pos_w, lm_plane, flags, equation, active, dist_thresh):
    """the numpy side of plp_plane_refine_points_host and its host build; returns (pos_w (M, 3), the new positions, changed (M,) u8)"""
    pw = np.array(pos_w, np.float64, order="C").reshape(-1, 3)
    M = len(pw)
    lp = np.ascontiguousarray(lm_plane, np.int32).reshape(M); fl = np.ascontiguousarray(flags, np.uint8).reshape(M)
    eq = np.ascontiguousarray(equation, np.float64).reshape(-1, 4); ac = np.ascontiguousarray(active, np.uint8).reshape(len(eq))
    th = np.array([dist_thresh], np.float64)
    ch = np.zeros(M, np.uint8)
    call(_struct(plane_refine_args_c, dict(M=M, NP=len(eq)), host_ptrs(pos_w=pw, lm_plane=lp, flags=fl, equation=eq, active=ac, dist_thresh=th, out_changed=ch)))
    return pw, ch


def model_plane_refine_points(pos_w, lm_plane, flags, equation, active, dist_thresh):
    """Host build of Planar_Mapping_module::refine_points (csrc/plane_fit.hpp, D19; no GPU needed): the arguments and result of
    matcher.plane_refine_points."""
    return _plane_refine_host(model_call("plp_model_plane_refine_points_host", "M"), pos_w, lm_plane, flags, equation, active, dist_thresh)


# the tables of plp_plane_refinement_*: name -> (shape per problem given (NP_cap, n_cap, L), dtype); all but lm_erased are updated in place
PLANE_REFINEMENT_TABLES = dict(pl_state=(lambda NP, M, L: (NP,), np.uint8), pl_equation=(lambda NP, M, L: (NP, 4), np.float64),
                               pl_best_error=(lambda NP, M, L: (NP,), np.float64), pl_count=(lambda NP, M, L: (NP,), np.int32),
                               pl_lm=(lambda NP, M, L: (NP, M), np.int32), pos_w=(lambda NP, M, L: (L, 3), np.float64),
                               lm_erased=(lambda NP, M, L: (L,), np.uint8), lm_owner=(lambda NP, M, L: (L,), np.int32))
# the outputs of plp_plane_refinement_*: name -> (shape per problem given (NP_cap, L, merge_cap), dtype)
PLANE_REFINEMENT_OUTPUTS = dict(status=(lambda NP, L, MC: (), np.uint8), was_merged=(lambda NP, L, MC: (), np.uint8),
                                planes_changed=(lambda NP, L, MC: (), np.uint8), points_changed=(lambda NP, L, MC: (), np.uint8),
                                removed=(lambda NP, L, MC: (NP,), np.uint8), num_merges=(lambda NP, L, MC: (), np.int32),
                                merges=(lambda NP, L, MC: (MC, 2), np.int32), num_updates=(lambda NP, L, MC: (), np.int32),
                                update_status=(lambda NP, L, MC: (NP,), np.uint8), lm_changed=(lambda NP, L, MC: (L,), np.uint8))


def _plane_refinement_host(call, tables, dist_thresh, error_thresh, points_per_ransac, iters, dot_product_threshold, offset_delta_factor, seed, stages,
                           merge_cap, out):
    """the numpy side of plp_plane_refinement_host and plp_model_plane_refinement_host: call(args struct) runs the entry.  tables: a dict of the
    arrays of PLANE_REFINEMENT_TABLES with a leading problem axis; an array of the right type is updated in place, anything else is replaced in
    the dict by the array that was."""
    st = np.asarray(tables["pl_state"])
    lm = np.asarray(tables["pl_lm"])
    if st.ndim != 2 or lm.ndim != 3 or lm.shape[:2] != st.shape:
        raise PlpError(PLP_ERR_INVALID_ARG, "pl_state must be (G, NP_cap) and pl_lm (G, NP_cap, n_cap)")
    G, NP = st.shape
    M = lm.shape[2]
    L = int(np.asarray(tables["lm_owner"]).reshape(G, -1).shape[1]) if G else 0
    t = {}
    for k, (shape, dt) in PLANE_REFINEMENT_TABLES.items():
        v = tables[k]
        if not (isinstance(v, np.ndarray) and v.dtype == dt and v.shape == (G,) + shape(NP, M, L) and v.flags.c_contiguous and v.flags.writeable):
            v = np.array(v, dt, order="C").reshape((G,) + shape(NP, M, L))
        t[k] = v
    vec = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (G,)))
    dt_, et_ = vec(dist_thresh), vec(error_thresh)
    MC = int(merge_cap)
    o = out_arrays(((k, (G,) + shape(NP, L, MC), dt) for k, (shape, dt) in PLANE_REFINEMENT_OUTPUTS.items()), out)
    a = _struct(plane_refinement_args_c, dict(G=G, NP_cap=NP, n_cap=M, L=L, merge_cap=MC, stages=int(stages), points_per_ransac=int(points_per_ransac),
                                              iters=int(iters), offset_delta_factor=int(offset_delta_factor), dot_product_threshold=float(dot_product_threshold),
                                              seed=int(seed) & 0xFFFFFFFFFFFFFFFF), host_ptrs(dist_thresh=dt_, error_thresh=et_, **t))
    set_outputs(a, PLANE_REFINEMENT_OUTPUTS, o, host_ptr)
    call(a)
    tables.update(t)
    return o


def model_plane_refinement(tables, dist_thresh, error_thresh, points_per_ransac=18, iters=50, dot_product_threshold=0.8, offset_delta_factor=6, seed=0,
                           stages=PLANE_STAGE_ALL, merge_cap=16, out=None):
    """Host build of Planar_Mapping_module::refinement() (csrc/plane_refinement.hpp; no GPU needed): the arguments and the
    result of matcher.plane_refinement."""
    return _plane_refinement_host(model_call("plp_model_plane_refinement_host", "G"), tables, dist_thresh, error_thresh, points_per_ransac, iters,
                                  dot_product_threshold, offset_delta_factor, seed, stages, merge_cap, out)


class planar_mapper:
    """Mirror of Planar_Mapping_module's plane fitting (planar_mapping_module.h) under the yaml's names: cfg maps "Threshold.iterationsCount",
    "Threshold.inliers_ratio_thr", "Threshold.min_number_points_before_ransac", "Threshold.point_per_ransac", "Threshold.plane_distance_correction"
    and "Threshold.final_error_correction" (load_configuration, :1162-1184; "Threshold.use_graph_cut" must be absent or false: that estimator
    needs a third-party library and is not offered).  mt: a matcher (the GPU entry), or None = the host build.  A plane is its landmark list:
    pos_w (n, 3), flags (n,) PLANE_LM_* bytes.  merge_planes, refine_planes, refinement and the table form of refine_points
    take the map's tables as a dict and need "Threshold.dot_product_threshold" and "Threshold.offset_delta_factor" (:1172-1173) as well."""

    def __init__(self, cfg, mt=None, seed=0):
        if cfg.get("Threshold.use_graph_cut", False):
            raise PlpError(PLP_ERR_UNSUPPORTED, "Threshold.use_graph_cut: estimate_plane_sequential_Graph_cut_RANSAC is not offered")
        self._iters = int(cfg["Threshold.iterationsCount"])
        self._ratio = float(cfg["Threshold.inliers_ratio_thr"])
        self._min_points = int(cfg["Threshold.min_number_points_before_ransac"])
        self._ppr = int(cfg["Threshold.point_per_ransac"])
        self._dist_corr = float(cfg["Threshold.plane_distance_correction"])
        self._err_corr = float(cfg["Threshold.final_error_correction"])
        self._mt, self._seed, self._cfg = mt, seed, cfg
        self.set_map_scale(1.0)

    def set_map_scale(self, map_scale):
        """estimate_map_scale (:130-183): _planar_distance_thresh and _final_error_thresh follow the scale"""
        self._map_scale = float(map_scale)
        self.planar_distance_thresh = self._dist_corr * self._map_scale
        self.final_error_thresh = self._err_corr * self._map_scale

    def _run(self, mode, pos_w, flags, samples, **kw):
        fl = np.asarray(flags, np.uint8).reshape(1, -1)
        fn = model_plane_ransac if self._mt is None else self._mt.plane_ransac
        r = fn(mode, np.asarray(pos_w, np.float64).reshape(1, fl.shape[1], 3), fl, self.planar_distance_thresh, self.final_error_thresh,
               points_per_ransac=self._ppr, min_points_before_ransac=self._min_points, iters=self._iters, inliers_ratio_thr=self._ratio,
               samples=None if samples is None else np.asarray(samples, np.int32)[None], seed=self._seed, **kw)
        return {k: v[0] for k, v in r.items()}

    def estimate_plane_sequential_RANSAC(self, pos_w, flags, samples=None):
        """create_new_plane's gate (:359) and estimate_plane_sequential_RANSAC (:412-591): the outputs of one problem; it returned true where
        status == PLANE_OK"""
        return self._run(PLANE_CREATE, pos_w, flags, samples)

    def update_plane_via_RANSAC(self, pos_w, flags, equation, best_error, samples=None):
        """update_plane_via_RANSAC (:593-733) of a plane with this equation and best error"""
        return self._run(PLANE_UPDATE, pos_w, flags, samples, equation_in=np.asarray(equation, np.float64).reshape(1, 4), best_error_in=[best_error])

    def refine_points(self, pos_w, lm_plane=None, flags=None, equation=None, active=None):
        """refine_points (:954-1004): (the new pos_w, changed).  With a dict of the map's tables (PLANE_REFINEMENT_TABLES) as the only argument:
        the function over the plane table, as merge_planes below"""
        if isinstance(pos_w, dict):
            return self._refinement(pos_w, PLANE_STAGE_REFINE_POINTS)
        fn = model_plane_refine_points if self._mt is None else self._mt.plane_refine_points
        return fn(pos_w, lm_plane, flags, equation, active, self.planar_distance_thresh)

    def _refinement(self, tables, stages, merge_cap=16, out=None):
        """plp_plane_refinement_* on the map's tables (one map: no problem axis; updated in place or replaced in the dict); grows n_cap and runs
        again from the tables as they were when a merge passes it (PLANE_REFINEMENT_OVERFLOW)"""
        if "Threshold.dot_product_threshold" not in self._cfg or "Threshold.offset_delta_factor" not in self._cfg:
            raise PlpError(PLP_ERR_INVALID_ARG, "Threshold.dot_product_threshold and Threshold.offset_delta_factor are required (load_configuration, :1172-1173)")
        fn = model_plane_refinement if self._mt is None else self._mt.plane_refinement
        while True:
            t = {k: np.array(tables[k], dt)[None] for k, (_, dt) in PLANE_REFINEMENT_TABLES.items()}
            r = fn(t, self.planar_distance_thresh, self.final_error_thresh, points_per_ransac=self._ppr, iters=self._iters,
                   dot_product_threshold=float(self._cfg["Threshold.dot_product_threshold"]), offset_delta_factor=int(self._cfg["Threshold.offset_delta_factor"]),
                   seed=self._seed, stages=stages, merge_cap=merge_cap, out=out)
            if int(r["status"][0]) != PLANE_REFINEMENT_OVERFLOW:
                break
            lm = np.asarray(tables["pl_lm"], np.int32)                        # the caller's tables are as they were: twice the slots
            tables["pl_lm"] = np.concatenate([lm, np.full((lm.shape[0], max(lm.shape[1], 1)), -1, np.int32)], axis=1)
        for k in PLANE_REFINEMENT_TABLES:
            tables[k] = t[k][0]
        return {k: v[0] for k, v in r.items()}

    def merge_planes(self, tables, merge_cap=16):
        """merge_planes (:795-898) over a dict of the map's tables: pl_state (NP,), pl_equation (NP, 4), pl_best_error, pl_count (NP,), pl_lm
        (NP, n_cap), pos_w (L, 3), lm_erased, lm_owner (L,).  Returns the outputs of one problem (PLANE_REFINEMENT_OUTPUTS); it returned true
        where was_merged"""
        return self._refinement(tables, PLANE_STAGE_MERGE, merge_cap)

    def refine_planes(self, tables):
        """refine_planes (:900-952) over the tables; it returned true where planes_changed"""
        return self._refinement(tables, PLANE_STAGE_REFINE_PLANES)

    def refinement(self, tables, merge_cap=16):
        """refinement() (:773-793) over the tables: the gate, merge_planes, refine_planes, refine_points"""
        return self._refinement(tables, PLANE_STAGE_ALL, merge_cap)


def model_sym_jacobi(A):
    """Host build of uses 1 and 2 of DESIGN.md section 5, D14 (csrc/pnp.hpp; no GPU needed): the one-sided Jacobi on symmetric positive
    semi-definite matrices.  A: (n, d, d) or (d, d) f64, d = 3 or 12.  Returns (vals (n, d) singular values descending, ut (n, d, d): row r =
    the vector of vals[r], sweeps (n,) i32: the sweeps that rotated, 60 = limit)."""
    A = np.ascontiguousarray(A, np.float64)
    single = A.ndim == 2
    d = A.shape[-1]
    A = A.reshape(-1, d * d)
    n = len(A)
    vals = np.zeros((n, d)); ut = np.zeros((n, d, d)); sw = np.zeros(n, np.int32)
    if lib().plp_model_sym_jacobi_host(host_ptr(A), d, n, host_ptr(vals), host_ptr(ut), host_ptr(sw)) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "A must be (n, 3, 3) or (n, 12, 12)")
    return (vals[0], ut[0], int(sw[0])) if single else (vals, ut, sw)


def model_lstsq6(A, b):
    """Host build of use 3 of D14 (csrc/pnp.hpp; no GPU needed): the minimum-norm least-squares solution of 6 x k systems, k = 3, 4, 5.
    A: (n, 6, k) or (6, k), b: (n, 6) or (6,).  Returns (x (n, k), sweeps (n,))."""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    single = A.ndim == 2
    k = A.shape[-1]
    A = A.reshape(-1, 6 * k); b = b.reshape(-1, 6)
    n = len(A)
    x = np.zeros((n, k)); sw = np.zeros(n, np.int32)
    if len(b) != n or lib().plp_model_lstsq6_host(host_ptr(A), host_ptr(b), k, n, host_ptr(x), host_ptr(sw)) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "A must be (n, 6, k) with k = 3, 4, 5 and b (n, 6)")
    return (x[0], int(sw[0])) if single else (x, sw)


def model_rot_from_abt(Abt):
    """Host build of use 4 of D14 (csrc/pnp.hpp; no GPU needed): R = U V^T of 3 x 3 matrices with the det < 0 flip of estimate_R_and_t
    (solve/pnp_solver.cc:487-514).  Abt: (n, 3, 3) or (3, 3).  Returns (R (n, 3, 3), sweeps (n,))."""
    A = np.ascontiguousarray(Abt, np.float64)
    single = A.ndim == 2
    A = A.reshape(-1, 9)
    n = len(A)
    R = np.zeros((n, 3, 3)); sw = np.zeros(n, np.int32)
    assert lib().plp_model_rot_from_abt_host(host_ptr(A), n, host_ptr(R), host_ptr(sw)) == n
    return (R[0], int(sw[0])) if single else (R, sw)


def model_epnp(pos_w, bearing, offsets=None):
    """Host build of pnp_solver::compute_pose (solve/pnp_solver.cc:230-290; csrc/pnp.hpp, D14; no GPU needed) for lists of correspondences:
    pos_w / bearing (m, 3) f64, list i = rows offsets[i] .. offsets[i+1] (None: one list of all rows).  Returns dict(rot (n, 3, 3), trans
    (n, 3), err (n,): the reprojection error, N (n,) i32: the chosen approximation 1 .. 3 (0: no correspondence left), sweeps (n, 8) i32);
    without the leading axis for offsets None."""
    w = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3); b = np.ascontiguousarray(bearing, np.float64).reshape(-1, 3)
    if len(w) != len(b):
        raise PlpError(PLP_ERR_INVALID_ARG, "pos_w and bearing must hold the same number of rows")
    single = offsets is None
    off = np.array([0, len(w)], np.int32) if single else np.ascontiguousarray(offsets, np.int32).reshape(-1)
    n = len(off) - 1
    if n < 0 or (n and int(off[-1]) > len(w)):
        raise PlpError(PLP_ERR_INVALID_ARG, "offsets must be ascending within the rows")
    o = dict(rot=np.zeros((n, 3, 3)), trans=np.zeros((n, 3)), err=np.zeros(n), N=np.zeros(n, np.int32), sweeps=np.zeros((n, 8), np.int32))
    if lib().plp_model_epnp_host(host_ptr(w), host_ptr(b), host_ptr(off), n, host_ptr(o["rot"]), host_ptr(o["trans"]), host_ptr(o["err"]),
                                 host_ptr(o["N"]), host_ptr(o["sweeps"])) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "offsets must be ascending within the rows")
    return {k: v[0] for k, v in o.items()} if single else o


def model_pnp_draw(seed, p, iters, num_matches, iter0=0):
    """The samples plp_pnp_ransac_* draw for problem p when the caller passes none (D14's generator; no GPU needed): (iters, 4) i32"""
    return model_draw("plp_model_pnp_draw_host", "num_matches must be at least 4, iters non-negative", seed, p, iters, iter0, 4, num_matches)


def model_pnp_thresholds(scale_factors):
    """max_cos_errors_ per level (solve/pnp_solver.cc:47-51): util::cos((float)(scale_factors[l] * (1.0 * M_PI / 180.0))), f32 (no GPU needed)"""
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    out = np.zeros(len(sf), np.float32)
    assert lib().plp_model_pnp_thresholds_host(host_ptr(sf), len(sf), host_ptr(out)) == len(sf)
    return out


# the outputs of plp_pnp_ransac_*: name -> (shape per problem given (n_cap, iters), dtype, optional)
PNP_OUTPUTS = dict(status=(lambda M, I: (), np.uint8, False), num_matches=(lambda M, I: (), np.int32, False), rot_cw=(lambda M, I: (3, 3), np.float64, False),
                   trans_cw=(lambda M, I: (3,), np.float64, False), num_inliers=(lambda M, I: (), np.int32, False),
                   best_iter=(lambda M, I: (), np.int32, False), inliers=(lambda M, I: (M,), np.uint8, True), hyp_inliers=(lambda M, I: (I,), np.int32, True))


def _pnp_ransac_host(call, valid, bearing, pos_w, octave, scale_factors, iters, min_num_inliers, recompute, samples, seed, counts, outputs, out):
    """the numpy side of plp_pnp_ransac_host and plp_model_pnp_ransac_host: call(args struct) runs the entry"""
    va = np.ascontiguousarray(valid, np.uint8)
    if va.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "valid must be (P, n_cap)")
    P_, M = va.shape
    be = np.ascontiguousarray(bearing, np.float64).reshape(P_, M, 3); pw = np.ascontiguousarray(pos_w, np.float64).reshape(P_, M, 3)
    oc = np.ascontiguousarray(octave, np.int32).reshape(P_, M)
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    I = int(iters)
    sm = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(P_, I, 4)
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(P_)
    o = out_arrays(((k, (P_,) + shape(M, max(I, 0)), dt) for k, (shape, dt, optional) in PNP_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    a = _struct(pnp_ransac_args_c, dict(P=P_, n_cap=M, min_num_inliers=int(min_num_inliers), iters=I, recompute=int(bool(recompute)),
                                        seed=int(seed) & 0xFFFFFFFFFFFFFFFF, num_levels=len(sf)), host_ptrs(
        scale_factors=sf, counts=cn, valid=va, bearing=be, pos_w=pw, octave=oc, samples=sm))
    set_outputs(a, PNP_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_pnp_ransac(valid, bearing, pos_w, octave, scale_factors, iters=30, min_num_inliers=10, recompute=True, samples=None, seed=0, counts=None,
                     outputs=None, out=None):
    """Host build of solve::pnp_solver's constructor and find_via_ransac (csrc/pnp.hpp; no GPU needed): the arguments
    and the result of matcher.pnp_ransac."""
    return _pnp_ransac_host(model_call("plp_model_pnp_ransac_host", "P"), valid, bearing, pos_w, octave, scale_factors, iters, min_num_inliers, recompute,
                            samples, seed, counts, outputs, out)


class pnp_solver:
    """Mirror of solve::pnp_solver (solve/pnp_solver.h): valid_bearings (n, 3), valid_keypts_octaves (n,) -- the octave is all the constructor
    reads of a key point --, valid_landmarks (n, 3), scale_factors.  mt: a matcher (the GPU entry), or None = the host build.  samples / seed:
    as matcher.pnp_ransac."""

    def __init__(self, valid_bearings, valid_keypts_octaves, valid_landmarks, scale_factors, min_num_inliers=10, mt=None, samples=None, seed=0):
        b = np.ascontiguousarray(valid_bearings, np.float64).reshape(-1, 3)
        n = len(b)
        self._n = n
        self._in = (np.ones((1, max(n, 1)), np.uint8), b.reshape(1, n, 3) if n else np.zeros((1, 1, 3)),
                    np.ascontiguousarray(valid_landmarks, np.float64).reshape(1, n, 3) if n else np.zeros((1, 1, 3)),
                    np.ascontiguousarray(valid_keypts_octaves, np.int32).reshape(1, n) if n else np.zeros((1, 1), np.int32), scale_factors)
        self._kw = dict(min_num_inliers=min_num_inliers, samples=samples, seed=seed, counts=np.array([n], np.int32))
        self._mt = mt
        self._r = None

    def find_via_ransac(self, max_num_iter, recompute=True):
        fn = model_pnp_ransac if self._mt is None else self._mt.pnp_ransac
        self._r = fn(*self._in, iters=int(max_num_iter), recompute=recompute, **self._kw)

    def solution_is_valid(self):
        return self._r is not None and int(self._r["status"][0]) == PNP_OK

    def get_best_rotation(self):
        return self._r["rot_cw"][0].copy()

    def get_best_translation(self):
        return self._r["trans_cw"][0].copy()

    def get_best_cam_pose(self):
        T = np.eye(4)
        T[:3, :3] = self._r["rot_cw"][0]
        T[:3, 3] = self._r["trans_cw"][0]
        return T

    def get_inlier_flags(self):
        return self._r["inliers"][0, :self._n].astype(bool)


# the outputs of plp_pose_optimize_*: name -> (shape per frame given (n_cap, l_cap, num_trials), dtype, optional)
POSE_OPT_OUTPUTS = dict(status=(lambda N, L, T: (), np.uint8, False), pose=(lambda N, L, T: (15,), np.float64, False),
                        num_init_obs=(lambda N, L, T: (), np.int32, False), num_valid=(lambda N, L, T: (), np.int32, False),
                        outlier=(lambda N, L, T: (N,), np.uint8, False), outlier_lines=(lambda N, L, T: (L,), np.uint8, False),
                        trial_info=(lambda N, L, T: (T, 4), np.int32, True), trial_chi2=(lambda N, L, T: (T, 2), np.float64, True))


def _pose_optimize_inputs(camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right, counts, lines, num_trials, num_each_iter):
    """the input half of a plp_pose_optimize_args from numpy arrays: (args struct, the arrays it points to, B, n_cap, l_cap)"""
    va = np.ascontiguousarray(valid, np.uint8)
    if va.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "valid must be (B, n_cap)")
    B, N = va.shape
    po = np.ascontiguousarray(pose_in, np.float64)
    if po.ndim != 2 or po.shape[0] != B or po.shape[1] < 12:
        raise PlpError(PLP_ERR_INVALID_ARG, "pose_in must be (B, 12 or more)")
    kp = np.ascontiguousarray(undist, KP_DTYPE).reshape(B, N); pw = np.ascontiguousarray(pos_w, np.float64).reshape(B, N, 3)
    xr = None if x_right is None else np.ascontiguousarray(x_right, np.float32).reshape(B, N)
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(B)
    sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
    L = 0; lv = kl = lw = lc = sl = None
    if lines is not None:
        lv = np.ascontiguousarray(lines["valid"], np.uint8).reshape(B, -1)
        L = lv.shape[1]
        kl = np.ascontiguousarray(lines["keylines"], KL_DTYPE).reshape(B, L); lw = np.ascontiguousarray(lines["pos_w"], np.float64).reshape(B, L, 6)
        lc = None if lines.get("counts") is None else np.ascontiguousarray(lines["counts"], np.int32).reshape(B)
        sl = np.ascontiguousarray(lines["inv_level_sigma_sq_lsd"], np.float32).reshape(-1)
    a = _struct(pose_optimize_args_c, dict(setup_type=int(setup_type), B=B, n_cap=N, l_cap=L, num_trials=int(num_trials), num_each_iter=int(num_each_iter),
                                           pose_stride=po.shape[1], num_levels=len(sg), num_levels_lsd=0 if sl is None else len(sl)), host_ptrs(
        inv_level_sigma_sq=sg, inv_level_sigma_sq_lsd=sl, pose_in=po, counts=cn, line_counts=lc, valid=va, undist=kp, x_right=xr, pos_w=pw, line_valid=lv,
        keylines=kl, pos_w_lines=lw))
    a.camera = camera_model_c.from_buffer_copy(camera)
    return a, (va, po, kp, pw, xr, cn, sg, lv, kl, lw, lc, sl), B, N, L


def _pose_optimize_host(call, camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right, counts, lines, num_trials, num_each_iter,
                        outputs, out):
    """the numpy side of plp_pose_optimize_host and plp_model_pose_optimize_host: call(args struct) runs the entry"""
    a, keep, B, N, L = _pose_optimize_inputs(camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right, counts, lines, num_trials,
                                             num_each_iter)
    o = out_arrays(((k, (B,) + shape(N, L, max(int(num_trials), 0)), dt) for k, (shape, dt, optional) in POSE_OPT_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, POSE_OPT_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_pose_optimize(camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right=None, counts=None, lines=None, num_trials=4,
                        num_each_iter=10, outputs=None, out=None):
    """Host build of optimize::pose_optimizer[_extended_line]::optimize (csrc/pose_opt.hpp; no GPU needed): the arguments
    and the result of matcher.pose_optimize."""
    return _pose_optimize_host(model_call("plp_model_pose_optimize_host", "B", neg_status=True), camera, setup_type, pose_in, valid, undist, pos_w,
                               inv_level_sigma_sq, x_right, counts, lines, num_trials, num_each_iter, outputs, out)


def model_pose_linearize(camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right=None, counts=None, lines=None, robust=True,
                         active=None, active_lines=None):
    """Host build of one linearisation of D15 at the poses pose_in (no GPU needed): the edges of the observation slots whose `active` /
    `active_lines` byte is set (None = all), Huber kernels on or off.  Returns dict(H (B, 21) upper triangle row-major, b (B, 6), chi2 (B,) the
    robust sum, edge_chi2 (B, n_cap), edge_chi2_lines (B, l_cap); NaN where no edge was evaluated)."""
    a, keep, B, N, L = _pose_optimize_inputs(camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right, counts, lines, 1, 1)
    ac = None if active is None else np.ascontiguousarray(active, np.uint8).reshape(B, N)
    al = None if active_lines is None else np.ascontiguousarray(active_lines, np.uint8).reshape(B, L)
    sums = np.zeros((B, 28)); ec = np.full((B, N), np.nan); el = np.full((B, L), np.nan)
    # the checks of the entry want its required outputs
    dummy = _pose_optimize_host(lambda a_: None, camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right, counts, lines, 1, 1, None, None)
    for k in ("status", "pose", "num_init_obs", "num_valid", "outlier", "outlier_lines"):
        setattr(a, "out_" + k, host_ptr(dummy[k]))
    r = lib().plp_model_pose_linearize_host(C.byref(a), int(bool(robust)), host_ptr(ac), host_ptr(al), host_ptr(sums), host_ptr(ec), host_ptr(el))
    if r != B:
        raise PlpError(-r, lib().plp_last_error().decode())
    return dict(H=sums[:, :21].copy(), b=sums[:, 21:27].copy(), chi2=sums[:, 27].copy(), edge_chi2=ec, edge_chi2_lines=el)


def model_se3_exp(update, est):
    """Host build of shot_vertex::oplusImpl (D15 item 1; no GPU needed): SE3Quat::exp(update) * est for n pairs; update (n, 6) = (omega, upsilon),
    est (n, 7) = (qx, qy, qz, qw, tx, ty, tz).  Returns (n, 7)."""
    u = np.ascontiguousarray(update, np.float64).reshape(-1, 6); e = np.ascontiguousarray(est, np.float64).reshape(-1, 7)
    assert len(u) == len(e)
    o = np.zeros_like(e)
    if lib().plp_model_se3_exp_host(_p(u), _p(e), len(u), _p(o)) != len(u):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_se3_exp_host")
    return o


def model_chol6(H, b, lam):
    """Host build of D15 item 4 (no GPU needed): (H + lambda I) x = b for n systems; H (n, 21) upper triangle row-major, b (n, 6), lam (n,).
    Returns (x (n, 6), ok (n,) bool); x is zero where a pivot was not positive and finite."""
    H = np.ascontiguousarray(H, np.float64).reshape(-1, 21); b = np.ascontiguousarray(b, np.float64).reshape(-1, 6)
    lam = np.ascontiguousarray(lam, np.float64).reshape(-1)
    assert len(H) == len(b) == len(lam)
    x = np.zeros_like(b); ok = np.zeros(len(H), np.int32)
    if lib().plp_model_chol6_host(_p(H), _p(b), _p(lam), len(H), _p(x), _p(ok)) != len(H):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_chol6_host")
    return x, ok.astype(bool)


def model_pose_sincos(x):
    """Host build of D15's sin and cos (csrc/pose_opt.hpp pose_sincos; no GPU needed; model_sincos is the line extractor's f32 pair): (sin, cos) f64"""
    x = np.ascontiguousarray(x, np.float64)
    s = np.zeros(x.shape); c = np.zeros(x.shape)
    if lib().plp_model_pose_sincos_host(_p(x), x.size, _p(s), _p(c)) != x.size:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_pose_sincos_host")
    return s, c


class pose_optimizer:
    """Mirror of optimize::pose_optimizer and optimize::pose_optimizer_extended_line (optimize/pose_optimizer.h): optimize() takes one frame's
    arrays and returns (num_valid, result dict of that frame); mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, num_trials=4, num_each_iter=10, mt=None):
        self.num_trials, self.num_each_iter, self._mt = int(num_trials), int(num_each_iter), mt

    def optimize(self, camera, setup_type, cam_pose_cw, valid, undist_keypts, pos_w, inv_level_sigma_sq, x_right=None, lines=None):
        """cam_pose_cw: 4 x 4 (or a 12 / 15-double pose row); valid (n,), undist_keypts (n,) KP_DTYPE, pos_w (n, 3); lines: None or dict(valid (l,),
        keylines (l,) KL_DTYPE, pos_w (l, 6), inv_level_sigma_sq_lsd).  Returns (the reference's return value, dict(status, pose (15,), cam_pose_cw
        4 x 4, num_init_obs, outlier (n,), outlier_lines (l,), trial_info, trial_chi2))."""
        T = np.asarray(cam_pose_cw, np.float64)
        row = np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]) if T.shape == (4, 4) else T.reshape(-1)[:12]
        n = len(np.asarray(valid).reshape(-1))
        ln = None if lines is None else dict(lines, valid=np.asarray(lines["valid"]).reshape(1, -1))
        fn = model_pose_optimize if self._mt is None else self._mt.pose_optimize
        r = fn(camera, setup_type, row.reshape(1, 12), np.asarray(valid).reshape(1, n), undist_keypts, pos_w, inv_level_sigma_sq, x_right=x_right, lines=ln,
               num_trials=self.num_trials, num_each_iter=self.num_each_iter)
        o = {k: v[0] for k, v in r.items()}
        M = np.eye(4); M[:3, :3] = o["pose"][:9].reshape(3, 3); M[:3, 3] = o["pose"][9:12]
        o["cam_pose_cw"] = M
        return int(o["num_valid"]), o


# the outputs of plp_transform_optimize_*: name -> (shape per problem given n_cap, dtype, optional); round_info[..., 3] is a POSE_OPT_END_*
TRANSFORM_OPT_OUTPUTS = dict(status=(lambda N: (), np.uint8, False), num_valid=(lambda N: (), np.int32, False), num_inliers=(lambda N: (), np.int32, False),
                             rot_12=(lambda N: (9,), np.float64, False), trans_12=(lambda N: (3,), np.float64, False), scale_12=(lambda N: (), np.float64, False),
                             world_to_1=(lambda N: (13,), np.float64, True), kept=(lambda N: (N,), np.uint8, False),
                             round_info=(lambda N: (2, 4), np.int32, True), round_chi2=(lambda N: (2, 2), np.float64, True))


def _transform_optimize_inputs(camera, fix_scale, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2, rot_12, trans_12, scale_12, inv_level_sigma_sq_1,
                               inv_level_sigma_sq_2, counts, num_iter, chi_sq):
    """the input half of a plp_transform_optimize_args from numpy arrays: (args struct, the arrays it points to, P, n_cap)"""
    va = np.ascontiguousarray(valid, np.uint8)
    if va.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "valid must be (P, n_cap)")
    P, N = va.shape
    w1 = np.ascontiguousarray(pos_w_1, np.float64).reshape(P, N, 3); w2 = np.ascontiguousarray(pos_w_2, np.float64).reshape(P, N, 3)
    k1 = np.ascontiguousarray(undist_1, KP_DTYPE).reshape(P, N); k2 = np.ascontiguousarray(undist_2, KP_DTYPE).reshape(P, N)
    p1 = np.ascontiguousarray(pose_1, np.float64).reshape(P, 15); p2 = np.ascontiguousarray(pose_2, np.float64).reshape(P, 15)
    r = np.ascontiguousarray(rot_12, np.float64).reshape(P, 9); t = np.ascontiguousarray(trans_12, np.float64).reshape(P, 3)
    sc = np.ascontiguousarray(scale_12, np.float32).reshape(P)
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(P)
    s1 = np.ascontiguousarray(inv_level_sigma_sq_1, np.float32).reshape(-1); s2 = np.ascontiguousarray(inv_level_sigma_sq_2, np.float32).reshape(-1)
    if len(s1) != len(s2):
        raise PlpError(PLP_ERR_INVALID_ARG, "the two sigma tables must have one length")
    a = _struct(transform_optimize_args_c, dict(fix_scale=int(bool(fix_scale)), num_iter=int(num_iter), chi_sq=float(chi_sq), P=P, n_cap=N, num_levels=len(s1)), host_ptrs(
        inv_level_sigma_sq_1=s1, inv_level_sigma_sq_2=s2, counts=cn, valid=va, pos_w_1=w1, pos_w_2=w2, undist_1=k1, undist_2=k2, pose_1=p1, pose_2=p2,
        rot_12=r, trans_12=t, scale_12=sc))
    a.camera = camera_model_c.from_buffer_copy(camera)
    return a, (va, w1, w2, k1, k2, p1, p2, r, t, sc, cn, s1, s2), P, N


def _transform_optimize_host(call, inputs, outputs, out):
    """the numpy side of plp_transform_optimize_host and plp_model_transform_optimize_host: call(args struct) runs the entry"""
    a, keep, P, N = _transform_optimize_inputs(**inputs)
    o = out_arrays(((k, (P,) + shape(N), dt) for k, (shape, dt, optional) in TRANSFORM_OPT_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, TRANSFORM_OPT_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_transform_optimize(camera, fix_scale, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2, rot_12, trans_12, scale_12, inv_level_sigma_sq_1,
                             inv_level_sigma_sq_2, counts=None, num_iter=10, chi_sq=10.0, outputs=None, out=None):
    """Host build of optimize::transform_optimizer::optimize (csrc/transform_opt.hpp; no GPU needed): the arguments and
    the result of matcher.transform_optimize."""
    call = model_call("plp_model_transform_optimize_host", "P", neg_status=True)
    inputs = dict(camera=camera, fix_scale=fix_scale, valid=valid, pos_w_1=pos_w_1, pos_w_2=pos_w_2, undist_1=undist_1, undist_2=undist_2, pose_1=pose_1,
                  pose_2=pose_2, rot_12=rot_12, trans_12=trans_12, scale_12=scale_12, inv_level_sigma_sq_1=inv_level_sigma_sq_1,
                  inv_level_sigma_sq_2=inv_level_sigma_sq_2, counts=counts, num_iter=num_iter, chi_sq=chi_sq)
    return _transform_optimize_host(call, inputs, outputs, out)


def model_transform_linearize(camera, fix_scale, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2, rot_12, trans_12, scale_12, inv_level_sigma_sq_1,
                              inv_level_sigma_sq_2, counts=None, chi_sq=10.0, active=None):
    """Host build of one linearisation of D16 at the Sim3 (rot_12, trans_12, scale_12) (no GPU needed): the two edges of every observation slot whose
    `active` byte is set (None = all).  Returns dict(H (P, 28) upper triangle row-major, b (P, 7), chi2 (P,) the robust sum, edge_chi2 (P, n_cap, 2)
    forward / backward; NaN where no edge was evaluated)."""
    inputs = dict(camera=camera, fix_scale=fix_scale, valid=valid, pos_w_1=pos_w_1, pos_w_2=pos_w_2, undist_1=undist_1, undist_2=undist_2, pose_1=pose_1,
                  pose_2=pose_2, rot_12=rot_12, trans_12=trans_12, scale_12=scale_12, inv_level_sigma_sq_1=inv_level_sigma_sq_1,
                  inv_level_sigma_sq_2=inv_level_sigma_sq_2, counts=counts, num_iter=1, chi_sq=chi_sq)
    a, keep, P, N = _transform_optimize_inputs(**inputs)
    ac = None if active is None else np.ascontiguousarray(active, np.uint8).reshape(P, N)
    sums = np.zeros((P, 36)); ec = np.full((P, N, 2), np.nan)
    r = lib().plp_model_transform_linearize_host(C.byref(a), host_ptr(ac), host_ptr(sums), host_ptr(ec))
    if r != P:
        raise PlpError(-r, lib().plp_last_error().decode())
    return dict(H=sums[:, :28].copy(), b=sums[:, 28:35].copy(), chi2=sums[:, 35].copy(), edge_chi2=ec)


def model_sim3_exp(update, est, fix_scale=False):
    """Host build of transform_vertex::oplusImpl (D16; no GPU needed): Sim3(update) * est for n pairs; update (n, 7) = (omega, upsilon, sigma), est
    (n, 8) = (qx, qy, qz, qw, tx, ty, tz, s).  Returns (n, 8)."""
    u = np.ascontiguousarray(update, np.float64).reshape(-1, 7); e = np.ascontiguousarray(est, np.float64).reshape(-1, 8)
    assert len(u) == len(e)
    o = np.zeros_like(e)
    if lib().plp_model_sim3_exp_host(_p(u), _p(e), int(bool(fix_scale)), len(u), _p(o)) != len(u):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_sim3_exp_host")
    return o


def model_chol7(H, b, lam):
    """Host build of the 7 x 7 solve of D16 (no GPU needed): (H + lambda I) x = b for n systems; H (n, 28) upper triangle row-major, b (n, 7), lam (n,).
    Returns (x (n, 7), ok (n,) bool); x is zero where a pivot was not positive and finite."""
    H = np.ascontiguousarray(H, np.float64).reshape(-1, 28); b = np.ascontiguousarray(b, np.float64).reshape(-1, 7)
    lam = np.ascontiguousarray(lam, np.float64).reshape(-1)
    assert len(H) == len(b) == len(lam)
    x = np.zeros_like(b); ok = np.zeros(len(H), np.int32)
    if lib().plp_model_chol7_host(_p(H), _p(b), _p(lam), len(H), _p(x), _p(ok)) != len(H):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_chol7_host")
    return x, ok.astype(bool)


def model_pose_exp(x):
    """Host build of D16's exp (csrc/transform_opt.hpp pose_exp; no GPU needed): f64, NaN outside [-700, 700]"""
    x = np.ascontiguousarray(x, np.float64)
    o = np.zeros(x.shape)
    if lib().plp_model_pose_exp_host(_p(x), x.size, _p(o)) != x.size:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_pose_exp_host")
    return o


class transform_optimizer:
    """Mirror of optimize::transform_optimizer (optimize/transform_optimizer.h): optimize() takes one pair's arrays and returns (num_inliers, result
    dict of that pair); mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, fix_scale, num_iter=10, mt=None):
        self.fix_scale, self.num_iter, self._mt = bool(fix_scale), int(num_iter), mt

    def optimize(self, camera, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2, rot_12, trans_12, scale_12, inv_level_sigma_sq_1,
                 inv_level_sigma_sq_2, chi_sq=10.0):
        """valid (n,): the slots that pass the four `continue`s of :95-118; pos_w_1 / pos_w_2 (n, 3), undist_1 / undist_2 (n,) KP_DTYPE, pose_1 / pose_2 15-double
        pose rows, (rot_12 3 x 3, trans_12, scale_12) the g2o::Sim3 to refine.  Returns (the reference's return value, dict(status, num_valid, rot_12 (9,),
        trans_12, scale_12, world_to_1 (13,), kept (n,): matched_lms_in_keyfrm_2 still set, round_info, round_chi2))."""
        n = len(np.asarray(valid).reshape(-1))
        fn = model_transform_optimize if self._mt is None else self._mt.transform_optimize
        r = fn(camera, self.fix_scale, np.asarray(valid).reshape(1, n), pos_w_1, pos_w_2, undist_1, undist_2, np.asarray(pose_1, np.float64).reshape(1, 15),
               np.asarray(pose_2, np.float64).reshape(1, 15), np.asarray(rot_12, np.float64).reshape(1, 9), np.asarray(trans_12, np.float64).reshape(1, 3),
               np.asarray(scale_12, np.float32).reshape(1), inv_level_sigma_sq_1, inv_level_sigma_sq_2, num_iter=self.num_iter, chi_sq=chi_sq)
        o = {k: v[0] for k, v in r.items()}
        return int(o["num_inliers"]), o


# the outputs of plp_local_ba_*: name -> (shape per problem given (F, L, T), dtype, optional); round_info[..., 3] is a POSE_OPT_END_* (0: round not run)
LOCAL_BA_OUTPUTS = dict(status=(lambda F, L, T: (), np.uint8, False), kf_role=(lambda F, L, T: (F,), np.uint8, False), lm_role=(lambda F, L, T: (L,), np.uint8, False),
                        pose=(lambda F, L, T: (F, 15), np.float64, False), pos_w=(lambda F, L, T: (L, 3), np.float64, False),
                        outlier=(lambda F, L, T: (T,), np.uint8, False), round_info=(lambda F, L, T: (2, 4), np.int32, True),
                        round_chi2=(lambda F, L, T: (2, 2), np.float64, True))


def _local_ba_inputs(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin,
                     lm_erased, num_first_iter, num_second_iter):
    """the input half of a plp_local_ba_args from numpy arrays: (args struct, the arrays it points to, G, F, L, T).  pose (F, pose_stride >= 12); undist / x_right
    (F, kp_stride): the row widths are the strides of the struct."""
    po = np.ascontiguousarray(pose, np.float64)
    if po.ndim != 2 or po.shape[1] < 12:
        raise PlpError(PLP_ERR_INVALID_ARG, "pose must be (F, pose_stride >= 12)")
    F = po.shape[0]
    ku = np.ascontiguousarray(undist, KP_DTYPE)
    ku = ku.reshape(F, -1) if F else ku.reshape(0, 0)
    K = ku.shape[1]
    xr = None if x_right is None else np.ascontiguousarray(x_right, np.float32).reshape(F, K)
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    L = len(pw)
    oo = np.ascontiguousarray(obs_offsets, np.int32).reshape(-1); ok = np.ascontiguousarray(obs_kf, np.int32).reshape(-1); oi = np.ascontiguousarray(obs_idx, np.int32).reshape(-1)
    if len(oo) != L + 1 or len(ok) != len(oi):
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_offsets must have L + 1 entries, obs_kf and obs_idx one length")
    T = len(ok)
    kl = np.ascontiguousarray(kf_local, np.uint8).reshape(-1, F) if F else np.zeros((np.asarray(kf_local).shape[0], 0), np.uint8)
    G = kl.shape[0]
    u8 = lambda v, n: None if v is None else np.ascontiguousarray(v, np.uint8).reshape(n)
    ke, ko, le = u8(kf_erased, F), u8(kf_is_origin, F), u8(lm_erased, L)
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
    sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
    a = _struct(local_ba_args_c, dict(setup_type=int(setup_type), num_first_iter=int(num_first_iter), num_second_iter=int(num_second_iter), G=G, F=F, L=L, T=T,
                                      kp_stride=int(K), pose_stride=po.shape[1], num_levels=len(sg)), host_ptrs(
        inv_level_sigma_sq=sg, pose=po, kf_erased=ke, kf_is_origin=ko, undist=ku, x_right=xr, counts=cn, pos_w=pw, lm_erased=le, obs_offsets=oo, obs_kf=ok,
        obs_idx=oi, kf_local=kl))
    a.camera = camera_model_c.from_buffer_copy(camera)
    return a, (po, ku, xr, pw, oo, ok, oi, kl, ke, ko, le, cn, sg), G, F, L, T


def _local_ba_host(call, inputs, outputs, out):
    """the numpy side of plp_local_ba_host and plp_model_local_ba_host: call(args struct) runs the entry"""
    a, keep, G, F, L, T = _local_ba_inputs(**inputs)
    o = out_arrays(((k, (G,) + shape(F, L, T), dt) for k, (shape, dt, optional) in LOCAL_BA_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, LOCAL_BA_OUTPUTS, o, host_ptr)
    call(a)
    return o


def _local_ba_kw(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin,
                 lm_erased, num_first_iter, num_second_iter):
    return dict(camera=camera, setup_type=setup_type, pose=pose, undist=undist, pos_w=pos_w, obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx,
                kf_local=kf_local, inv_level_sigma_sq=inv_level_sigma_sq, x_right=x_right, counts=counts, kf_erased=kf_erased, kf_is_origin=kf_is_origin,
                lm_erased=lm_erased, num_first_iter=num_first_iter, num_second_iter=num_second_iter)


def model_local_ba(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right=None, counts=None,
                   kf_erased=None, kf_is_origin=None, lm_erased=None, num_first_iter=5, num_second_iter=10, outputs=None, out=None):
    """Host build of optimize::local_bundle_adjuster::optimize (csrc/local_ba.hpp; no GPU needed): the arguments and the
    result of matcher.local_ba."""
    return _local_ba_host(model_call("plp_model_local_ba_host", "G", neg_status=True), _local_ba_kw(
        camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin, lm_erased,
        num_first_iter, num_second_iter), outputs, out)


def model_local_ba_linearize(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right=None, counts=None,
                             kf_erased=None, kf_is_origin=None, lm_erased=None, robust=True):
    """Host build of one linearisation of D17 at the inputs' estimates, every edge at level 0 (no GPU needed); kf_local (F,) or (1, F).  Returns
    dict(free_kf (P,) table rows of the active free key frames, Hpp (P, 21) upper triangle row-major, bp (P, 6), Hll (L, 6) (00 01 02 11 12 22) and bl (L, 3),
    NaN for a landmark without an edge, W (T, 6, 3) NaN where the edge has no active free pose, chi2 the robust sum, edge_chi2 (T,) NaN where no edge)."""
    a, keep, G, F, L, T = _local_ba_inputs(**_local_ba_kw(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq,
                                                          x_right, counts, kf_erased, kf_is_origin, lm_erased, 1, 1))
    fk = np.full(LOCAL_BA_MAX_FREE, -1, np.int32); hpp = np.full((LOCAL_BA_MAX_FREE, 27), np.nan); hll = np.full((L, 9), np.nan); w = np.full((T, 18), np.nan)
    chi = np.zeros(1); ec = np.full(T, np.nan)
    r = lib().plp_model_local_ba_linearize_host(C.byref(a), int(bool(robust)), host_ptr(fk), host_ptr(hpp), host_ptr(hll), host_ptr(w), host_ptr(chi), host_ptr(ec))
    if r < 0:
        raise PlpError(-r, lib().plp_last_error().decode())
    return dict(free_kf=fk[:r].copy(), Hpp=hpp[:r, :21].copy(), bp=hpp[:r, 21:].copy(), Hll=hll[:, :6].copy(), bl=hll[:, 6:].copy(), W=w.reshape(T, 6, 3),
                chi2=float(chi[0]), edge_chi2=ec)


def model_local_ba_solve(Hpp, bp, Hll, bl, e_pose, e_lm, W, lam):
    """Host build of one damped Schur solve of D17 (no GPU needed): Hpp (P, 21), bp (P, 6), Hll (M, 6), bl (M, 3), edges in landmark order with e_pose (E,)
    (-1: a constant pose), e_lm (E,) and W (E, 6, 3).  Returns (x_p (P, 6), x_l (M, 3), ok)."""
    hp = np.concatenate([np.asarray(Hpp, np.float64).reshape(-1, 21), np.asarray(bp, np.float64).reshape(-1, 6)], axis=1).copy()
    hl = np.concatenate([np.asarray(Hll, np.float64).reshape(-1, 6), np.asarray(bl, np.float64).reshape(-1, 3)], axis=1).copy()
    ep = np.ascontiguousarray(e_pose, np.int32).reshape(-1); el = np.ascontiguousarray(e_lm, np.int32).reshape(-1)
    w = np.ascontiguousarray(W, np.float64).reshape(len(ep), 18)
    xp = np.zeros((len(hp), 6)); xl = np.zeros((len(hl), 3))
    r = lib().plp_model_local_ba_solve_host(len(hp), len(hl), len(ep), *map(host_ptr, (hp, hl, ep, el, w)), float(lam), host_ptr(xp), host_ptr(xl))
    if r < 0:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_local_ba_solve_host")
    return xp, xl, bool(r)


def model_inv3(a):
    """Host build of D17's closed 3 x 3 inverse (no GPU needed): a (n, 6) symmetric (00 01 02 11 12 22).  Returns (inverse (n, 6), ok (n,) bool)."""
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 6)
    o = np.zeros_like(a); ok = np.zeros(len(a), np.int32)
    if lib().plp_model_inv3_host(_p(a), len(a), _p(o), _p(ok)) != len(a):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_inv3_host")
    return o, ok.astype(bool)


class local_bundle_adjuster:
    """Mirror of optimize::local_bundle_adjuster (optimize/local_bundle_adjuster.h): optimize() takes the map tables and one problem's kf_local and
    returns that problem's result dict; mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, num_first_iter=5, num_second_iter=10, mt=None):
        self.num_first_iter, self.num_second_iter, self._mt = int(num_first_iter), int(num_second_iter), mt

    def optimize(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right=None, counts=None,
                 kf_erased=None, kf_is_origin=None, lm_erased=None):
        """kf_local (F,): the current key frame and its covisibilities (:73-91).  Returns dict(status, kf_role (F,), lm_role (L,), pose (F, 15), pos_w (L, 3),
        outlier (T,), round_info, round_chi2); rows the adjuster does not write are zero."""
        fn = model_local_ba if self._mt is None else self._mt.local_ba
        r = fn(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, np.asarray(kf_local, np.uint8).reshape(1, -1), inv_level_sigma_sq,
               x_right=x_right, counts=counts, kf_erased=kf_erased, kf_is_origin=kf_is_origin, lm_erased=lm_erased, num_first_iter=self.num_first_iter,
               num_second_iter=self.num_second_iter)
        return {k: v[0] for k, v in r.items()}


# the outputs plp_local_ba_lines_* adds to LOCAL_BA_OUTPUTS: name -> (shape per problem given (LL, TL), dtype)
LOCAL_BA_LINES_OUTPUTS = dict(line_role=(lambda LL, TL: (LL,), np.uint8), pluecker=(lambda LL, TL: (LL, 6), np.float64), outlier_lines=(lambda LL, TL: (TL,), np.uint8))


def _local_ba_lines_inputs(points, keylines, pluecker, obs_offsets_lines, obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, kl_counts, line_erased):
    """the input half of a plp_local_ba_lines_args: `points` the keywords of _local_ba_inputs; (args struct, the arrays it points to, G, F, L, T, LL, TL)"""
    pa, keep, G, F, L, T = _local_ba_inputs(**points)
    kl = np.ascontiguousarray(keylines, KL_DTYPE)
    kl = kl.reshape(F, -1) if F else kl.reshape(0, 0)
    pk = np.ascontiguousarray(pluecker, np.float64).reshape(-1, 6)
    LL = len(pk)
    oo = np.ascontiguousarray(obs_offsets_lines, np.int32).reshape(-1); ok = np.ascontiguousarray(obs_kf_lines, np.int32).reshape(-1)
    oi = np.ascontiguousarray(obs_idx_lines, np.int32).reshape(-1)
    if len(oo) != LL + 1 or len(ok) != len(oi):
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_offsets_lines must have LL + 1 entries, obs_kf_lines and obs_idx_lines one length")
    TL = len(ok)
    kc = None if kl_counts is None else np.ascontiguousarray(kl_counts, np.int32).reshape(F)
    le = None if line_erased is None else np.ascontiguousarray(line_erased, np.uint8).reshape(LL)
    sg = np.ascontiguousarray(inv_level_sigma_sq_lsd, np.float32).reshape(-1)
    a = _struct(local_ba_lines_args_c, dict(LL=LL, TL=TL, kl_stride=int(kl.shape[1]), num_levels_lsd=len(sg)), host_ptrs(
        inv_level_sigma_sq_lsd=sg, keylines=kl, kl_counts=kc, pluecker=pk, line_erased=le, obs_offsets_lines=oo, obs_kf_lines=ok, obs_idx_lines=oi))
    a.points = pa
    return a, (keep, kl, pk, oo, ok, oi, kc, le, sg), G, F, L, T, LL, TL


def _local_ba_lines_host(call, inputs, outputs, out):
    """the numpy side of plp_local_ba_lines_host and plp_model_local_ba_lines_host: call(args struct) runs the entry"""
    a, keep, G, F, L, T, LL, TL = _local_ba_lines_inputs(**inputs)
    o = out_arrays([(k, (G,) + shape(F, L, T), dt) for k, (shape, dt, optional) in LOCAL_BA_OUTPUTS.items() if wanted(k, optional, outputs)] +
                   [(k, (G,) + shape(LL, TL), dt) for k, (shape, dt) in LOCAL_BA_LINES_OUTPUTS.items()], out)
    set_outputs(a.points, LOCAL_BA_OUTPUTS, o, host_ptr)
    set_outputs(a, LOCAL_BA_LINES_OUTPUTS, o, host_ptr)
    call(a)
    return o


def _local_ba_lines_kw(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, keylines, pluecker, obs_offsets_lines,
                       obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, x_right, counts, kf_erased, kf_is_origin, lm_erased, kl_counts, line_erased,
                       num_first_iter, num_second_iter):
    return dict(points=_local_ba_kw(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right, counts, kf_erased,
                                    kf_is_origin, lm_erased, num_first_iter, num_second_iter),
                keylines=keylines, pluecker=pluecker, obs_offsets_lines=obs_offsets_lines, obs_kf_lines=obs_kf_lines, obs_idx_lines=obs_idx_lines,
                inv_level_sigma_sq_lsd=inv_level_sigma_sq_lsd, kl_counts=kl_counts, line_erased=line_erased)


def _model_lines_call(a):
    r = lib().plp_model_local_ba_lines_host(C.byref(a))
    if r != a.points.G:
        raise PlpError(-r, lib().plp_last_error().decode())


def model_local_ba_lines(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, keylines, pluecker, obs_offsets_lines,
                         obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, x_right=None, counts=None, kf_erased=None, kf_is_origin=None, lm_erased=None,
                         kl_counts=None, line_erased=None, num_first_iter=5, num_second_iter=10, outputs=None, out=None):
    """Host build of optimize::local_bundle_adjuster_extended_line::optimize (csrc/local_ba_lines.hpp; no GPU needed): the
    arguments and the result of matcher.local_ba_lines."""
    return _local_ba_lines_host(_model_lines_call, _local_ba_lines_kw(
        camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, keylines, pluecker, obs_offsets_lines, obs_kf_lines,
        obs_idx_lines, inv_level_sigma_sq_lsd, x_right, counts, kf_erased, kf_is_origin, lm_erased, kl_counts, line_erased, num_first_iter, num_second_iter),
        outputs, out)


def model_line_oplus(line, update):
    """Host build of D28's Line3D::oplus (no GPU needed): line (n, 6) Pluecker (m, d), update (n, 4).  Returns (n, 6)."""
    ln = np.ascontiguousarray(line, np.float64).reshape(-1, 6); up = np.ascontiguousarray(update, np.float64).reshape(-1, 4)
    o = np.zeros_like(ln)
    if len(ln) != len(up) or lib().plp_model_line_oplus_host(_p(ln), _p(up), len(ln), _p(o)) != len(ln):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_line_oplus_host")
    return o


def model_local_ba_lines_linearize(robust=True, **kw):
    """Host build of one linearisation of D28 at the inputs' estimates, every edge at level 0 (no GPU needed); the keywords of model_local_ba_lines with
    kf_local (F,) or (1, F).  Returns model_local_ba_linearize's dict without W and edge_chi2, and Hnn (LL, 10) upper triangle row-major, bn (LL, 4), NaN for
    a line without an edge, W_lines (TL, 6, 4) NaN where the edge has no active free pose, edge_chi2_lines (TL,) NaN where no edge."""
    full = dict(x_right=None, counts=None, kf_erased=None, kf_is_origin=None, lm_erased=None, kl_counts=None, line_erased=None, num_first_iter=1, num_second_iter=1)
    full.update(kw)
    a, keep, G, F, L, T, LL, TL = _local_ba_lines_inputs(**_local_ba_lines_kw(**full))
    fk = np.full(LOCAL_BA_MAX_FREE, -1, np.int32); hpp = np.full((LOCAL_BA_MAX_FREE, 27), np.nan); hll = np.full((L, 9), np.nan); hnn = np.full((LL, 14), np.nan)
    w = np.full((TL, 24), np.nan); chi = np.zeros(1); ec = np.full(TL, np.nan)
    r = lib().plp_model_local_ba_lines_linearize_host(C.byref(a), int(bool(robust)), *map(host_ptr, (fk, hpp, hll, hnn, w, chi, ec)))
    if r < 0:
        raise PlpError(-r, lib().plp_last_error().decode())
    return dict(free_kf=fk[:r].copy(), Hpp=hpp[:r, :21].copy(), bp=hpp[:r, 21:].copy(), Hll=hll[:, :6].copy(), bl=hll[:, 6:].copy(), Hnn=hnn[:, :10].copy(),
                bn=hnn[:, 10:].copy(), W_lines=w.reshape(TL, 6, 4), chi2=float(chi[0]), edge_chi2_lines=ec)


def model_local_ba_lines_solve(Hpp, bp, Hll, bl, Hnn, bn, e_pose, e_lm, W, e_pose_lines, e_line, W_lines, lam):
    """Host build of one damped Schur solve of D28 with mixed 3- and 4-blocks (no GPU needed): model_local_ba_solve's arguments, and Hnn (N, 10), bn (N, 4),
    the line edges in line order with e_pose_lines (-1: a constant pose), e_line and W_lines (E4, 6, 4).  Returns (x_p (P, 6), x_l (M, 3), x_n (N, 4), ok)."""
    hp = np.concatenate([np.asarray(Hpp, np.float64).reshape(-1, 21), np.asarray(bp, np.float64).reshape(-1, 6)], axis=1).copy()
    hl = np.concatenate([np.asarray(Hll, np.float64).reshape(-1, 6), np.asarray(bl, np.float64).reshape(-1, 3)], axis=1).copy()
    hn = np.concatenate([np.asarray(Hnn, np.float64).reshape(-1, 10), np.asarray(bn, np.float64).reshape(-1, 4)], axis=1).copy()
    ep = np.ascontiguousarray(e_pose, np.int32).reshape(-1); el = np.ascontiguousarray(e_lm, np.int32).reshape(-1)
    eq = np.ascontiguousarray(e_pose_lines, np.int32).reshape(-1); en = np.ascontiguousarray(e_line, np.int32).reshape(-1)
    w = np.ascontiguousarray(W, np.float64).reshape(len(ep), 18); wn = np.ascontiguousarray(W_lines, np.float64).reshape(len(eq), 24)
    xp = np.zeros((len(hp), 6)); xl = np.zeros((len(hl), 3)); xn = np.zeros((len(hn), 4))
    r = lib().plp_model_local_ba_lines_solve_host(len(hp), len(hl), len(hn), len(ep), len(eq), *map(host_ptr, (hp, hl, hn, ep, el, w, eq, en, wn)), float(lam),
                                                  *map(host_ptr, (xp, xl, xn)))
    if r < 0:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_local_ba_lines_solve_host")
    return xp, xl, xn, bool(r)


class local_bundle_adjuster_extended_line:
    """Mirror of optimize::local_bundle_adjuster_extended_line (optimize/local_bundle_adjuster_extended_line.h): optimize() takes the map tables with the
    line tables and one problem's kf_local and returns that problem's result dict; mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, num_first_iter=5, num_second_iter=10, mt=None):
        self.num_first_iter, self.num_second_iter, self._mt = int(num_first_iter), int(num_second_iter), mt

    def optimize(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, keylines, pluecker, obs_offsets_lines,
                 obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, **optional):
        """kf_local (F,).  Returns local_bundle_adjuster.optimize's dict and line_role (LL,), pluecker (LL, 6), outlier_lines (TL,); rows the adjuster does not
        write are zero.  optional: x_right, counts, kf_erased, kf_is_origin, lm_erased, kl_counts, line_erased."""
        fn = model_local_ba_lines if self._mt is None else self._mt.local_ba_lines
        r = fn(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, np.asarray(kf_local, np.uint8).reshape(1, -1), inv_level_sigma_sq, keylines,
               pluecker, obs_offsets_lines, obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, num_first_iter=self.num_first_iter,
               num_second_iter=self.num_second_iter, **optional)
        return {k: v[0] for k, v in r.items()}


# the outputs of plp_pose_graph_optimize_*: name -> (shape per problem given (F, edge_cap), dtype, optional)
POSE_GRAPH_OUTPUTS = dict(status=(lambda F, E: (), np.uint8, False), num_edges=(lambda F, E: (), np.int32, True), edges=(lambda F, E: (E, 3), np.int32, True),
                          sim3_cw=(lambda F, E: (F, 8), np.float64, True), corrected_wc=(lambda F, E: (F, 8), np.float64, True),
                          pose=(lambda F, E: (F, 15), np.float64, True), info=(lambda F, E: (4,), np.int32, True), chi2=(lambda F, E: (2,), np.float64, True))
POSE_GRAPH_TABLES = ("pose", "kf_erased", "kf_id", "kf_parent", "kf_conn", "kf_conn_w", "kf_n_conn", "kf_covis", "kf_covis_w", "kf_n_covis", "kf_loop_offsets",
                     "kf_loop")


def _sim3_list(problems, key):
    """the CSR of a per-problem {row: Sim3} mapping, rows ascending: (offsets (G + 1,), rows, sims (n, 8))"""
    off, rows, sims = [0], [], []
    for pr in problems:
        for r, v in sorted((pr.get(key) or {}).items()):
            rows.append(int(r)); sims.append(np.asarray(v, np.float64).reshape(8))
        off.append(len(rows))
    return np.asarray(off, np.int32), np.asarray(rows, np.int32), np.asarray(sims, np.float64).reshape(-1, 8)


def pose_graph_problems(problems):
    """The per-problem arrays of a plp_pose_graph_args from a list of dicts(loop_kf, curr_kf, fix_scale=False, pre_corrected={row: Sim3}, non_corrected={row:
    Sim3}, loop_connections={owner row: set of rows}): the mappings become lists in ascending row, the library's order."""
    lc_off, lo, lt = [0], [], []
    for pr in problems:
        for a, targets in sorted((pr.get("loop_connections") or {}).items()):
            for b in sorted(targets):
                lo.append(int(a)); lt.append(int(b))
        lc_off.append(len(lo))
    po, pr_, ps = _sim3_list(problems, "pre_corrected")
    no, nr, ns = _sim3_list(problems, "non_corrected")
    return dict(loop_kf=np.asarray([p["loop_kf"] for p in problems], np.int32), curr_kf=np.asarray([p["curr_kf"] for p in problems], np.int32),
                fix_scale=np.asarray([bool(p.get("fix_scale")) for p in problems], np.uint8), pre_offsets=po, pre_row=pr_, pre_sim3=ps, non_offsets=no, non_row=nr,
                non_sim3=ns, lc_offsets=np.asarray(lc_off, np.int32), lc_owner=np.asarray(lo, np.int32), lc_target=np.asarray(lt, np.int32))


def _pose_graph_inputs(tables, problems, edge_cap, env_cap, max_iter):
    """the input half of a plp_pose_graph_args from numpy arrays: (args struct, the arrays it points to, G, F)"""
    po = np.ascontiguousarray(tables["pose"], np.float64)
    if po.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "pose must be (F, pose_stride)")
    F = po.shape[0]
    i32 = lambda v, shape: np.ascontiguousarray(v, np.int32).reshape(shape)
    t = dict(pose=po, kf_erased=None if tables.get("kf_erased") is None else np.ascontiguousarray(tables["kf_erased"], np.uint8).reshape(F),
             kf_id=i32(tables["kf_id"] if tables.get("kf_id") is not None else np.arange(F), F), kf_parent=i32(tables["kf_parent"], F),
             kf_conn=i32(tables["kf_conn"], (F, -1)) if F else np.zeros((0, 0), np.int32), kf_n_conn=i32(tables["kf_n_conn"], F),
             kf_covis=i32(tables["kf_covis"], (F, -1)) if F else np.zeros((0, 0), np.int32), kf_n_covis=i32(tables["kf_n_covis"], F))
    t["kf_conn_w"] = i32(tables["kf_conn_w"], t["kf_conn"].shape); t["kf_covis_w"] = i32(tables["kf_covis_w"], t["kf_covis"].shape)
    if tables.get("kf_loop_offsets") is not None:
        t["kf_loop_offsets"] = i32(tables["kf_loop_offsets"], F + 1); t["kf_loop"] = i32(tables["kf_loop"], -1)
        if len(t["kf_loop"]) == 0:
            t["kf_loop"] = np.zeros(1, np.int32)
    pr = problems if isinstance(problems, dict) else pose_graph_problems(problems)
    pr = {k: np.ascontiguousarray(v) for k, v in pr.items()}
    for k in ("pre_row", "pre_sim3", "non_row", "non_sim3", "lc_owner", "lc_target"):          # lists without an entry: the arrays are still required
        if pr[k].size == 0:
            pr[k] = np.zeros(8, pr[k].dtype)
    G = len(pr["loop_kf"])
    a = _struct(pose_graph_args_c, dict(G=G, F=F, pose_stride=po.shape[1], conn_cap=t["kf_conn"].shape[1], covis_cap=t["kf_covis"].shape[1], edge_cap=int(edge_cap),
                                        env_cap=int(env_cap), max_iter=int(max_iter)), {**{k: host_ptr(v) for k, v in t.items()}, **{k: host_ptr(v) for k, v in pr.items()}})
    return a, (t, pr), G, F


def _pose_graph_host(call, tables, problems, edge_cap, env_cap, max_iter, outputs, out):
    """the numpy side of plp_pose_graph_optimize_host and the host builds: call(args struct) runs the entry"""
    a, keep, G, F = _pose_graph_inputs(tables, problems, edge_cap, env_cap, max_iter)
    o = out_arrays(((k, (G,) + shape(F, int(edge_cap)), dt) for k, (shape, dt, optional) in POSE_GRAPH_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, POSE_GRAPH_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_pose_graph_optimize(tables, problems, edge_cap=POSE_GRAPH_MAX_EDGES, env_cap=POSE_GRAPH_MAX_ENV, max_iter=50, outputs=None, out=None):
    """Host build of optimize::graph_optimizer::optimize (csrc/pose_graph.hpp; no GPU needed): the arguments and the result
    of matcher.pose_graph_optimize."""
    return _pose_graph_host(model_call("plp_model_pose_graph_optimize_host", "G", neg_status=True), tables, problems, edge_cap, env_cap, max_iter, outputs, out)


def model_pose_graph_edges(tables, problems, edge_cap=POSE_GRAPH_MAX_EDGES, out=None):
    """Host build of D22's vertices and edge list alone (:85-298; no GPU needed): dict(status, num_edges, edges (G, edge_cap, 3), sim3_cw (G, F, 8))"""
    return _pose_graph_host(model_call("plp_model_pose_graph_edges_host", "G", neg_status=True), tables, problems, edge_cap, 1, 0,
                            ("num_edges", "edges", "sim3_cw"), out)


def model_sim3_log(sim3):
    """Host build of g2o's Sim3::log as D22 restates it (no GPU needed): sim3 (n, 8) or (8,) -> (n, 7) or (7,): omega, upsilon, sigma"""
    a = np.ascontiguousarray(sim3, np.float64)
    single = a.ndim == 1
    a = a.reshape(-1, 8)
    o = np.zeros((len(a), 7))
    if lib().plp_model_sim3_log_host(host_ptr(a), len(a), host_ptr(o)) != len(a):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_sim3_log_host")
    return o[0] if single else o


def model_pose_log(x):
    """Host build of D22's log (no GPU needed): NaN outside 1e-300 <= x <= 1e300"""
    a = np.ascontiguousarray(x, np.float64).reshape(-1)
    o = np.zeros_like(a)
    if lib().plp_model_pose_log_host(host_ptr(a), len(a), host_ptr(o)) != len(a):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_pose_log_host")
    return o


def model_pose_acos(x):
    """Host build of D22's acos (no GPU needed): NaN outside -1 <= x <= 1"""
    a = np.ascontiguousarray(x, np.float64).reshape(-1)
    o = np.zeros_like(a)
    if lib().plp_model_pose_acos_host(host_ptr(a), len(a), host_ptr(o)) != len(a):
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_pose_acos_host")
    return o


def pose_graph_envelope(H, first):
    """The skyline of a dense symmetric (7 n, 7 n) matrix in D22's layout: row block i holds the column blocks first[i] .. i as seven rows of 7 (i - first[i] + 1)"""
    H = np.asarray(H, np.float64)
    return np.concatenate([H[7 * i:7 * i + 7, 7 * int(f):7 * i + 7].reshape(-1) for i, f in enumerate(first)]) if len(first) else np.zeros(0)


def model_block_chol7(H, first, b, lam):
    """Host build of D22's block skyline solve (no GPU needed): (H + lam I) x = b for a dense symmetric H whose row block i is zero before column block
    first[i].  Returns (x (7 n,), ok)."""
    fi = np.ascontiguousarray(first, np.int32).reshape(-1)
    env = pose_graph_envelope(H, fi); bb = np.ascontiguousarray(b, np.float64).reshape(-1)
    x = np.zeros(7 * len(fi))
    r = lib().plp_model_block_chol7_host(len(fi), host_ptr(fi), host_ptr(env), host_ptr(bb), float(lam), host_ptr(x))
    if r < 0:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_block_chol7_host")
    return x, bool(r)


def _correct_landmarks_host(call, pos_w, ref_kf, sim3_cw, corrected_wc, lm_erased, kf_erased, out):
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3); L = len(pw)
    cw = np.ascontiguousarray(sim3_cw, np.float64).reshape(-1, 8); wc = np.ascontiguousarray(corrected_wc, np.float64).reshape(-1, 8); F = len(cw)
    rk = np.ascontiguousarray(ref_kf, np.int32).reshape(L)
    le = None if lm_erased is None else np.ascontiguousarray(lm_erased, np.uint8).reshape(L)
    ke = None if kf_erased is None else np.ascontiguousarray(kf_erased, np.uint8).reshape(F)
    o = dict(pos_w=(out or {}).get("pos_w"), status=(out or {}).get("status"))
    o["pos_w"] = np.zeros((L, 3)) if o["pos_w"] is None else o["pos_w"]
    o["status"] = np.zeros(L, np.uint8) if o["status"] is None else o["status"]
    if o["pos_w"].shape != (L, 3) or o["pos_w"].dtype != np.float64 or o["status"].shape != (L,) or o["status"].dtype != np.uint8:
        raise PlpError(PLP_ERR_INVALID_ARG, "out['pos_w'] must be (L, 3) f64, out['status'] (L,) u8")
    a = _struct(correct_landmarks_args_c, dict(L=L, F=F), host_ptrs(pos_w=pw, lm_erased=le, ref_kf=rk, kf_erased=ke, sim3_cw=cw, corrected_wc=wc,
                                                                    out_pos_w=o["pos_w"], out_status=o["status"]))
    call(a)
    return o


def model_correct_landmarks(pos_w, ref_kf, sim3_cw, corrected_wc, lm_erased=None, kf_erased=None, out=None):
    """Host build of the landmark half of graph_optimizer::optimize (:331-350; no GPU needed): the arguments and the result of matcher.correct_landmarks"""
    return _correct_landmarks_host(model_call("plp_model_correct_landmarks_host", "L"), pos_w, ref_kf, sim3_cw, corrected_wc, lm_erased, kf_erased, out)


class graph_optimizer:
    """Mirror of optimize::graph_optimizer (optimize/graph_optimizer.h): the map is the key-frame and graph tables (POSE_GRAPH_TABLES), optimize() takes the
    rows of the loop and the current key frame and the three mappings of the reference by row; mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, tables, fix_scale, mt=None, edge_cap=POSE_GRAPH_MAX_EDGES, env_cap=POSE_GRAPH_MAX_ENV):
        self.tables, self.fix_scale, self._mt, self.edge_cap, self.env_cap = tables, bool(fix_scale), mt, int(edge_cap), int(env_cap)

    def optimize(self, loop_kf, curr_kf, non_corrected, pre_corrected, loop_connections):
        """non_corrected / pre_corrected: {row: Sim3 (8,)}, loop_connections: {row: set of rows}.  Returns dict(status, num_edges, edges, sim3_cw (F, 8),
        corrected_wc (F, 8), pose (F, 15), info, chi2); rows that are no vertices are zero."""
        fn = model_pose_graph_optimize if self._mt is None else self._mt.pose_graph_optimize
        r = fn(self.tables, [dict(loop_kf=loop_kf, curr_kf=curr_kf, fix_scale=self.fix_scale, non_corrected=non_corrected, pre_corrected=pre_corrected,
                                  loop_connections=loop_connections)], edge_cap=self.edge_cap, env_cap=self.env_cap)
        return {k: v[0] for k, v in r.items()}
LOCAL_MAP_INPUTS = ("kf_erased", "kf_covis", "kf_parent", "kf_children_offsets", "kf_children", "kf_lm", "kf_counts", "kf_lm_lines", "kf_kl_counts",
                    "obs_offsets", "obs_kf", "lm_erased", "lm_erased_lines", "frm_lm", "frm_counts", "frm_lm_lines", "frm_kl_counts")


# the outputs of plp_local_map_*: name -> (which of k_cap / m_cap / ml_cap is its row length or None, dtype, optional, line side only)
LOCAL_MAP_OUTPUTS = dict(status=(None, np.uint8, False, False), num_first=(None, np.int32, False, False), num_kf=(None, np.int32, False, False),
                         local_kf=("k_cap", np.int32, False, False), first_weight=("k_cap", np.int32, True, False),
                         nearest_kf=(None, np.int32, False, False), num_lm=(None, np.int32, False, False), local_lm=("m_cap", np.int32, False, False),
                         held=("m_cap", np.uint8, False, False), num_lines=(None, np.int32, False, True),
                         local_lines=("ml_cap", np.int32, False, True), held_lines=("ml_cap", np.uint8, False, True))


def _local_map_host(call, kf_covis, kf_parent, kf_children_offsets, kf_children, kf_lm, obs_offsets, obs_kf, frm_lm, k_cap, m_cap, ml_cap, kf_erased, kf_counts,
                    kf_lm_lines, kf_kl_counts, lm_erased, lm_erased_lines, LL, frm_counts, frm_lm_lines, frm_kl_counts, max_num_local_keyfrms, workspace_bytes,
                    fcap, flcap, outputs, out):
    """the numpy side of plp_local_map_host and plp_model_local_map_host: call(args struct) runs the entry.  The row widths of kf_lm, kf_lm_lines,
    frm_lm and frm_lm_lines are cap, lcap and the two frame strides; fcap / flcap (default: the stride) are the slots read of a frame's row."""
    i32 = lambda v: array_or_none(v, np.int32)
    u8 = lambda v: array_or_none(v, np.uint8, -1)
    kp = i32(kf_parent).reshape(-1)
    F = len(kp)
    rows = lambda v, n: None if v is None else (i32(v).reshape(n, -1) if n else np.zeros((0, 0), np.int32))
    kc = rows(kf_covis, F)
    if F and kc.shape[1] != 10:
        raise PlpError(PLP_ERR_INVALID_ARG, "kf_covis must be (F, 10)")
    co, ch = i32(kf_children_offsets).reshape(-1), i32(kf_children).reshape(-1)
    kl, kll = rows(kf_lm, F), rows(kf_lm_lines, F)
    oo, ok = i32(obs_offsets).reshape(-1), i32(obs_kf).reshape(-1)
    fl = i32(frm_lm)
    if fl.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "frm_lm must be (B, stride)")
    B = fl.shape[0]
    fll = None if frm_lm_lines is None else i32(frm_lm_lines).reshape(B, -1)
    if len(co) != F + 1 or len(oo) < 1:
        raise PlpError(PLP_ERR_INVALID_ARG, "kf_children_offsets must have F + 1 entries, obs_offsets L + 1")
    L = len(oo) - 1
    le, lel = u8(lm_erased), u8(lm_erased_lines)
    LL = int(LL) if LL is not None else (len(lel) if lel is not None else 0)
    ke, kcn, kkc, fc, fkc = u8(kf_erased), i32(kf_counts), i32(kf_kl_counts), i32(frm_counts), i32(frm_kl_counts)
    for name, v, n in (("kf_erased", ke, F), ("kf_counts", kcn, F), ("kf_kl_counts", kkc, F), ("lm_erased", le, L), ("lm_erased_lines", lel, LL),
                       ("frm_counts", fc, B), ("frm_kl_counts", fkc, B)):
        if v is not None and v.size != n:
            raise PlpError(PLP_ERR_INVALID_ARG, f"{name} must have {n} entries")
    caps = dict(k_cap=int(k_cap), m_cap=int(m_cap), ml_cap=int(ml_cap))
    lines = kll is not None
    a = _struct(local_map_args_c, dict(B=B, F=F, C=len(ch), L=L, LL=LL, T=len(ok), cap=kl.shape[1], lcap=kll.shape[1] if lines else 0,
                                       fcap=fl.shape[1] if fcap is None else int(fcap), flcap=(fll.shape[1] if fll is not None else 0) if flcap is None else int(flcap),
                                       frm_stride=fl.shape[1], frm_stride_lines=fll.shape[1] if fll is not None else 0,
                                       max_num_local_keyfrms=int(max_num_local_keyfrms), workspace_bytes=int(workspace_bytes), **caps), host_ptrs(
        kf_erased=ke, kf_covis=kc, kf_parent=kp, kf_children_offsets=co, kf_children=ch, kf_lm=kl, kf_counts=kcn, kf_kl_counts=kkc, obs_offsets=oo, obs_kf=ok,
        lm_erased=le, lm_erased_lines=lel, frm_lm=fl, frm_counts=fc, frm_lm_lines=fll, frm_kl_counts=fkc))
    if lines:      # a table without a slot is still "line tracking is on": the pointer only has to be non-NULL
        a.kf_lm_lines = kll.ctypes.data if kll.size else kp.ctypes.data if kp.size else co.ctypes.data
    o = out_arrays(((k, (B,) if cap_name is None else (B, max(caps[cap_name], 0)), dt)      # a negative cap is the library's to refuse
                    for k, (cap_name, dt, optional, line_side) in LOCAL_MAP_OUTPUTS.items() if (lines or not line_side) and wanted(k, optional, outputs)), out)
    set_outputs(a, o, o, host_ptr)
    call(a)
    return o


def model_local_map(kf_covis, kf_parent, kf_children_offsets, kf_children, kf_lm, obs_offsets, obs_kf, frm_lm, k_cap, m_cap, ml_cap=0, kf_erased=None,
                    kf_counts=None, kf_lm_lines=None, kf_kl_counts=None, lm_erased=None, lm_erased_lines=None, LL=None, frm_counts=None, frm_lm_lines=None,
                    frm_kl_counts=None, max_num_local_keyfrms=60, workspace_bytes=0, fcap=None, flcap=None, outputs=None, out=None):
    """Host build of module::local_map_updater for B frames (csrc/local_map.hpp; no GPU needed): the arguments and the
    result of matcher.local_map."""
    return _local_map_host(model_call("plp_model_local_map_host", "B", neg_status=True), kf_covis, kf_parent, kf_children_offsets, kf_children, kf_lm,
                           obs_offsets, obs_kf, frm_lm, k_cap, m_cap, ml_cap, kf_erased, kf_counts, kf_lm_lines, kf_kl_counts, lm_erased, lm_erased_lines, LL,
                           frm_counts, frm_lm_lines, frm_kl_counts, max_num_local_keyfrms, workspace_bytes, fcap, flcap, outputs, out)


def kf_landmarks_from_observations(obs_offsets, obs_kf, obs_idx, F, cap):
    """kf_lm [F, cap] i32 from the observation lists (torch tensors on one device): slot (obs_kf[t], obs_idx[t]) takes the landmark whose run holds
    entry t, every other slot -1.  For callers whose keyframe landmarks_ and landmark observations_ agree (one landmark per slot); entries outside
    the table are left out.  Static shapes, no synchronisation."""
    import torch
    T, dev = obs_kf.shape[0], obs_kf.device
    out = torch.full((F * cap + 1,), -1, dtype=torch.int32, device=dev)
    if T == 0 or F * cap == 0:
        return out[:F * cap].view(F, cap)
    lm = torch.searchsorted(obs_offsets[1:].to(torch.int64).contiguous(), torch.arange(T, device=dev), right=True)
    kf, ix = obs_kf.to(torch.int64), obs_idx.to(torch.int64)
    inside = (kf >= 0) & (kf < F) & (ix >= 0) & (ix < cap)
    out.index_copy_(0, torch.where(inside, kf * cap + ix, torch.full_like(kf, F * cap)), lm.to(torch.int32))
    out[F * cap] = -1
    return out[:F * cap].view(F, cap)


class local_map_updater:
    """Mirror of module::local_map_updater (module/local_map_updater.h) for one frame: acquire_local_map() takes the map tables (a dict with the
    keys of LOCAL_MAP_INPUTS but the frm_* ones) and the frame's landmarks_ as rows; mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, max_num_local_keyfrms=60, mt=None):
        self.max_num_local_keyfrms, self._mt, self._r = int(max_num_local_keyfrms), mt, None

    def acquire_local_map(self, tables, frm_lm, frm_lm_lines=None, k_cap=None, m_cap=None, ml_cap=None, LL=None):
        """True iff a key frame voted (:60-66).  The caps default to what always fits: F key frames, L landmarks, LL lines."""
        F, L = len(np.asarray(tables["kf_parent"]).reshape(-1)), len(np.asarray(tables["obs_offsets"]).reshape(-1)) - 1
        lel = tables.get("lm_erased_lines")
        LL = int(LL) if LL is not None else (len(lel) if lel is not None else 0)
        fn = model_local_map if self._mt is None else self._mt.local_map
        opt = {k: tables.get(k) for k in ("kf_erased", "kf_counts", "kf_lm_lines", "kf_kl_counts", "lm_erased", "lm_erased_lines")}
        r = fn(tables["kf_covis"], tables["kf_parent"], tables["kf_children_offsets"], tables["kf_children"], tables["kf_lm"], tables["obs_offsets"],
               tables["obs_kf"], np.asarray(frm_lm, np.int32).reshape(1, -1), F if k_cap is None else k_cap, L if m_cap is None else m_cap,
               LL if ml_cap is None else ml_cap, LL=LL, frm_lm_lines=None if frm_lm_lines is None else np.asarray(frm_lm_lines, np.int32).reshape(1, -1),
               max_num_local_keyfrms=self.max_num_local_keyfrms, **opt)
        self._r = {k: v[0] for k, v in r.items()}
        return int(self._r["status"]) != LOCAL_MAP_NO_KEYFRAMES

    def get_local_keyframes(self):
        return self._r["local_kf"][:min(int(self._r["num_kf"]), len(self._r["local_kf"]))].copy()

    def get_local_landmarks(self):
        return self._r["local_lm"][:min(int(self._r["num_lm"]), len(self._r["local_lm"]))].copy()

    def get_local_landmarks_line(self):
        if "num_lines" not in self._r:
            return np.zeros(0, np.int32)
        return self._r["local_lines"][:min(int(self._r["num_lines"]), len(self._r["local_lines"]))].copy()

    def get_nearest_covisibility(self):
        """the key-frame row, or -1 where the reference's member is indeterminate (D18)"""
        return int(self._r["nearest_kf"])
CULL_KEYFRAMES_INPUTS = ("kf_lm", "kf_counts", "undist", "x_right", "depths", "depth_thr", "kf_id", "kf_erased", "kf_cannot_erase", "obs_offsets",
                         "obs_kf", "obs_idx", "lm_erased", "lm_num_obs", "cur_kf", "covis_offsets", "covis")


# the outputs of plp_cull_keyframes_*: name -> (shape from (G, Cv, F, L), dtype, optional)
CULL_KEYFRAMES_OUTPUTS = dict(num_removed=(lambda G, Cv, F, L: (G,), np.int32, False), decision=(lambda G, Cv, F, L: (Cv,), np.uint8, False),
                              num_valid=(lambda G, Cv, F, L: (Cv,), np.int32, False), num_redundant=(lambda G, Cv, F, L: (Cv,), np.int32, False),
                              kf_removed=(lambda G, Cv, F, L: (G, F), np.uint8, True), lm_erased=(lambda G, Cv, F, L: (G, L), np.uint8, True))
CULL_LANDMARKS_INPUTS = ("fresh_offsets", "fresh", "lm_erased", "num_observed", "num_observable", "first_kf_id", "num_obs", "owning_plane",
                         "cur_kf_id", "num_obs_thr")


# the outputs of plp_cull_landmarks_*: name -> (per entry (N) or per list (R), dtype)
CULL_LANDMARKS_OUTPUTS = dict(state=("N", np.uint8), num_removed=("R", np.int32), num_fresh=("R", np.int32), fresh=("N", np.int32))


def _cull_out(spec_items, out, a):
    """the output arrays of a culling entry: the caller's where given (unwritten slots keep their values), zeros otherwise"""
    o = out_arrays(spec_items, out)
    set_outputs(a, o, o, host_ptr)
    return o


def _cull_keyframes_host(call, kf_lm, undist, kf_id, obs_offsets, obs_kf, obs_idx, cur_kf, covis_offsets, covis, origin_id, is_monocular, kf_counts,
                         x_right, depths, depth_thr, kf_erased, kf_cannot_erase, lm_erased, lm_num_obs, outputs, out):
    """the numpy side of plp_cull_keyframes_host and plp_model_cull_keyframes_host: call(args struct) runs the entry.  The row widths of kf_lm and
    of undist (with x_right and depths) are cap and kp_stride."""
    i32 = lambda v: array_or_none(v, np.int32)
    u32 = lambda v: array_or_none(v, np.uint32, -1)
    u8 = lambda v: array_or_none(v, np.uint8, -1)
    kid = u32(kf_id)
    F = len(kid)
    kl = i32(kf_lm).reshape(F, -1) if F else np.zeros((0, 0), np.int32)
    un = np.ascontiguousarray(undist)
    if un.dtype != KP_DTYPE:
        un = np.ascontiguousarray(un, np.uint8).reshape(F, -1).view(KP_DTYPE)
    un = un.reshape(F, -1) if F else np.zeros((0, 0), KP_DTYPE)
    cap, stride = kl.shape[1], un.shape[1]
    f32 = lambda v, shape: None if v is None else np.ascontiguousarray(v, np.float32).reshape(shape)
    xr, dp, dt_ = f32(x_right, (F, stride)), f32(depths, (F, stride)), f32(depth_thr, (F,))
    oo, ok, oi = i32(obs_offsets).reshape(-1), i32(obs_kf).reshape(-1), i32(obs_idx).reshape(-1)
    ck, co, cv = i32(cur_kf).reshape(-1), i32(covis_offsets).reshape(-1), i32(covis).reshape(-1)
    if len(oo) < 1 or len(co) != len(ck) + 1 or len(oi) != len(ok):
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_offsets must have L + 1 entries, covis_offsets G + 1, obs_idx as many as obs_kf")
    L, G, Cv = len(oo) - 1, len(ck), len(cv)
    kcn, ke, kce, le, ln = i32(kf_counts), u8(kf_erased), u8(kf_cannot_erase), u8(lm_erased), u32(lm_num_obs)
    for name, v, n in (("kf_counts", kcn, F), ("kf_erased", ke, F), ("kf_cannot_erase", kce, F), ("lm_erased", le, L), ("lm_num_obs", ln, L)):
        if v is not None and v.size != n:
            raise PlpError(PLP_ERR_INVALID_ARG, f"{name} must have {n} entries")
    a = _struct(cull_keyframes_args_c, dict(F=F, L=L, T=len(ok), cap=cap, kp_stride=stride, G=G, Cv=Cv, origin_id=int(origin_id),
                                            is_monocular=int(bool(is_monocular))),
                host_ptrs(kf_lm=kl, kf_counts=kcn, undist=un, x_right=xr, depths=dp, depth_thr=dt_, kf_id=kid, kf_erased=ke, kf_cannot_erase=kce,
                          obs_offsets=oo, obs_kf=ok, obs_idx=oi, lm_erased=le, lm_num_obs=ln, cur_kf=ck, covis_offsets=co, covis=cv))
    o = _cull_out(((k, shape(G, Cv, F, L), dt) for k, (shape, dt, optional) in CULL_KEYFRAMES_OUTPUTS.items() if wanted(k, optional, outputs)), out, a)
    call(a)
    return o


def model_cull_keyframes(kf_lm, undist, kf_id, obs_offsets, obs_kf, obs_idx, cur_kf, covis_offsets, covis, origin_id=0, is_monocular=True,
                         kf_counts=None, x_right=None, depths=None, depth_thr=None, kf_erased=None, kf_cannot_erase=None, lm_erased=None,
                         lm_num_obs=None, outputs=None, out=None):
    """Host build of local_map_cleaner::remove_redundant_keyframes for G problems (csrc/map_cull.hpp; no GPU needed): the
    arguments and the result of matcher.cull_keyframes."""
    return _cull_keyframes_host(model_call("plp_model_cull_keyframes_host", "G", neg_status=True), kf_lm, undist, kf_id, obs_offsets, obs_kf, obs_idx, cur_kf,
                                covis_offsets, covis, origin_id, is_monocular, kf_counts, x_right, depths, depth_thr, kf_erased, kf_cannot_erase, lm_erased,
                                lm_num_obs, outputs, out)


def _cull_landmarks_host(call, fresh_offsets, fresh, num_observed, num_observable, first_kf_id, num_obs, cur_kf_id, num_obs_thr, lm_erased, owning_plane,
                         out):
    """the numpy side of plp_cull_landmarks_host and plp_model_cull_landmarks_host"""
    i32 = lambda v: np.ascontiguousarray(v, np.int32).reshape(-1)
    u32 = lambda v: np.ascontiguousarray(v, np.uint32).reshape(-1)
    u8 = lambda v: array_or_none(v, np.uint8, -1)
    fo, fr = i32(fresh_offsets), i32(fresh)
    nd, nb, fk, no, ck, th = u32(num_observed), u32(num_observable), u32(first_kf_id), u32(num_obs), u32(cur_kf_id), u32(num_obs_thr)
    L, R, N = len(nd), len(ck), len(fr)
    le, pl = u8(lm_erased), u8(owning_plane)
    if len(fo) != R + 1 or len(th) != R or any(len(v) != L for v in (nb, fk, no)) or any(v is not None and len(v) != L for v in (le, pl)):
        raise PlpError(PLP_ERR_INVALID_ARG, "fresh_offsets must have R + 1 entries, num_obs_thr R, every landmark table L")
    a = _struct(cull_landmarks_args_c, dict(R=R, N=N, L=L),
                host_ptrs(fresh_offsets=fo, fresh=fr, lm_erased=le, num_observed=nd, num_observable=nb, first_kf_id=fk, num_obs=no, owning_plane=pl,
                          cur_kf_id=ck, num_obs_thr=th))
    o = _cull_out([(k, (N,) if per == "N" else (R,), dt) for k, (per, dt) in CULL_LANDMARKS_OUTPUTS.items()], out, a)
    call(a)
    return o


def model_cull_landmarks(fresh_offsets, fresh, num_observed, num_observable, first_kf_id, num_obs, cur_kf_id, num_obs_thr, lm_erased=None,
                         owning_plane=None, out=None):
    """Host build of local_map_cleaner::remove_redundant_landmarks[_line] for R fresh lists (csrc/map_cull.hpp, D20; no GPU needed): the arguments
    and the result of matcher.cull_landmarks."""
    return _cull_landmarks_host(model_call("plp_model_cull_landmarks_host", "R", neg_status=True), fresh_offsets, fresh, num_observed, num_observable,
                                first_kf_id, num_obs, cur_kf_id, num_obs_thr, lm_erased, owning_plane, out)


class local_map_cleaner:
    """Mirror of module::local_map_cleaner (module/local_map_cleaner.h) over table rows: the fresh buffers hold landmark rows, the key frames are
    rows of the map tables the calls take.  mt: a matcher (the GPU entries), or None = the host build."""

    def __init__(self, is_monocular, mt=None):
        self.is_monocular, self._mt, self.origin_keyfrm_id = bool(is_monocular), mt, 0
        self.reset()

    def set_origin_keyframe_id(self, id_):
        self.origin_keyfrm_id = int(id_)

    def add_fresh_landmark(self, lm):
        self.fresh_landmarks.append(int(lm))

    def add_fresh_landmark_line(self, lm_line):
        self.fresh_landmarks_line.append(int(lm_line))

    def reset(self):
        self.fresh_landmarks, self.fresh_landmarks_line, self.last = [], [], None

    def _landmarks(self, fresh, cur_keyfrm_id, thr, tables, plane):
        fn = model_cull_landmarks if self._mt is None else self._mt.cull_landmarks
        r = fn([0, len(fresh)], fresh, tables["num_observed"], tables["num_observable"], tables["first_kf_id"], tables["num_obs"], [cur_keyfrm_id], [thr],
               lm_erased=tables.get("lm_erased"), owning_plane=tables.get("owning_plane") if plane else None)
        self.last = r
        return [int(v) for v in r["fresh"][:int(r["num_fresh"][0])]], int(r["num_removed"][0])

    def remove_redundant_landmarks(self, cur_keyfrm_id, tables):
        """tables: a dict of the per-row tables of CULL_LANDMARKS_INPUTS for the point landmarks.  Returns num_removed; self.last["state"] names
        what became of every entry (CULL_ERASE: the caller runs prepare_for_erasing() on it), fresh_landmarks keeps the HOLD ones."""
        self.fresh_landmarks, n = self._landmarks(self.fresh_landmarks, cur_keyfrm_id, 2 if self.is_monocular else 3, tables, True)
        return n

    def remove_redundant_landmarks_line(self, cur_keyfrm_id, tables):
        """the same for the line buffer, whose threshold is 3 and whose landmarks own no plane"""
        self.fresh_landmarks_line, n = self._landmarks(self.fresh_landmarks_line, cur_keyfrm_id, 3, tables, False)
        return n

    def remove_redundant_keyframes(self, cur_row, covisibilities, tables):
        """cur_row: the table row of cur_keyfrm; covisibilities: the rows of its get_covisibilities(), in order; tables: a dict with the keys of
        CULL_KEYFRAMES_INPUTS but the problem's.  Returns num_removed; self.last holds the outputs of CULL_KEYFRAMES_OUTPUTS (decision: which rows
        the caller runs prepare_for_erasing() on; kf_removed, lm_erased: the map afterwards)."""
        fn = model_cull_keyframes if self._mt is None else self._mt.cull_keyframes
        cv = np.asarray(covisibilities, np.int32).reshape(-1)
        opt = {k: tables.get(k) for k in ("kf_counts", "x_right", "depths", "depth_thr", "kf_erased", "kf_cannot_erase", "lm_erased", "lm_num_obs")}
        r = fn(tables["kf_lm"], tables["undist"], tables["kf_id"], tables["obs_offsets"], tables["obs_kf"], tables["obs_idx"], [int(cur_row)], [0, len(cv)],
               cv, origin_id=self.origin_keyfrm_id, is_monocular=self.is_monocular, **opt)
        self.last = r
        return int(r["num_removed"][0])
COVISIBILITY_INPUTS = ("kf_lm", "kf_counts", "obs_offsets", "obs_kf", "lm_erased", "kf_id", "owners")
# the state tables of plp_covisibility_*: name -> (row length from (conn_cap, covis_cap) or None, dtype, what an empty row holds)
COVISIBILITY_STATE = dict(kf_conn=(lambda cc, vc: cc, np.int32, -1), kf_conn_w=(lambda cc, vc: cc, np.int32, 0), kf_n_conn=(None, np.int32, 0),
                          kf_covis=(lambda cc, vc: vc, np.int32, -1), kf_covis_w=(lambda cc, vc: vc, np.int32, 0), kf_n_covis=(None, np.int32, 0),
                          kf_parent=(None, np.int32, -1), kf_parent_unset=(None, np.uint8, 1))
COVISIBILITY_ERASE_STATE = ("kf_conn", "kf_conn_w", "kf_n_conn", "kf_covis", "kf_covis_w", "kf_n_covis")
# the outputs of plp_covisibility_update_*: name -> (per owner (G) or per key frame (F), dtype, optional); plp_covisibility_erase_* has status
# and touched, both per key frame
COVISIBILITY_OUTPUTS = dict(status=("G", np.uint8, False), nearest=("G", np.int32, True), max_weight=("G", np.int32, True),
                            touched=("F", np.uint8, True))


def covisibility_state(F, conn_cap, covis_cap):
    """the state tables of F key frames without a connection, as numpy arrays"""
    return {k: np.full((F,) if row is None else (F, row(conn_cap, covis_cap)), fill, dt) for k, (row, dt, fill) in COVISIBILITY_STATE.items()}


def _covisibility_state_ptrs(state, names, F):
    """the caller's state tables as they are (the entry updates them in place): checked, and their pointers with the two caps"""
    for k in names:
        row, dt, _ = COVISIBILITY_STATE[k]
        v = state.get(k)
        if not (isinstance(v, np.ndarray) and v.dtype == dt and v.flags.c_contiguous and v.flags.writeable and v.shape[0] == F
                and v.ndim == (1 if row is None else 2)):
            raise PlpError(PLP_ERR_INVALID_ARG, f"state[{k!r}] must be a writeable C-contiguous {np.dtype(dt).name} array with a row per key frame")
    cc, vc = state["kf_conn"].shape[1], state["kf_covis"].shape[1]
    if state["kf_conn_w"].shape[1] != cc or state["kf_covis_w"].shape[1] != vc:
        raise PlpError(PLP_ERR_INVALID_ARG, "kf_conn_w and kf_covis_w must have the row lengths of kf_conn and kf_covis")
    return cc, vc, {k: host_ptr(state[k]) for k in names}


def _covisibility_update_host(call, kf_lm, obs_offsets, obs_kf, kf_id, state, owners, kf_counts, lm_erased, outputs, out):
    """the numpy side of plp_covisibility_update_host and plp_model_covisibility_update_host: call(args struct) runs the entry"""
    i32 = lambda v: array_or_none(v, np.int32)
    kid = np.ascontiguousarray(kf_id, np.uint32).reshape(-1)
    F = len(kid)
    kl = i32(kf_lm).reshape(F, -1) if F else np.zeros((0, 0), np.int32)
    oo, ok, ow = i32(obs_offsets).reshape(-1), i32(obs_kf).reshape(-1), i32(owners).reshape(-1)
    if len(oo) < 1:
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_offsets must have L + 1 entries")
    L, G = len(oo) - 1, len(ow)
    kcn = None if kf_counts is None else i32(kf_counts).reshape(-1)
    le = None if lm_erased is None else np.ascontiguousarray(lm_erased, np.uint8).reshape(-1)
    for name, v, n in (("kf_counts", kcn, F), ("lm_erased", le, L)):
        if v is not None and v.size != n:
            raise PlpError(PLP_ERR_INVALID_ARG, f"{name} must have {n} entries")
    cc, vc, sp = _covisibility_state_ptrs(state, COVISIBILITY_STATE, F)
    a = _struct(covisibility_update_args_c, dict(F=F, L=L, T=len(ok), cap=kl.shape[1], conn_cap=cc, covis_cap=vc, G=G),
                dict(sp, **host_ptrs(kf_lm=kl, kf_counts=kcn, obs_offsets=oo, obs_kf=ok, lm_erased=le, kf_id=kid, owners=ow)))
    o = _cull_out(((k, (G,) if per == "G" else (F,), dt) for k, (per, dt, optional) in COVISIBILITY_OUTPUTS.items() if wanted(k, optional, outputs)), out, a)
    call(a)
    return o


def _covisibility_erase_host(call, state, erased, out):
    """the numpy side of plp_covisibility_erase_host and plp_model_covisibility_erase_host"""
    er = np.ascontiguousarray(erased, np.uint8).reshape(-1)
    F = len(er)
    cc, vc, sp = _covisibility_state_ptrs(state, COVISIBILITY_ERASE_STATE, F)
    a = _struct(covisibility_erase_args_c, dict(F=F, conn_cap=cc, covis_cap=vc), dict(sp, erased=host_ptr(er)))
    o = _cull_out([("status", (F,), np.uint8), ("touched", (F,), np.uint8)], out, a)
    call(a)
    return o


def model_covisibility_update(kf_lm, obs_offsets, obs_kf, kf_id, state, owners, kf_counts=None, lm_erased=None, outputs=None, out=None):
    """Host build of graph_node::update_connections for a list of owners (csrc/covisibility.hpp; no GPU needed): the
    arguments and the result of matcher.covisibility_update."""
    return _covisibility_update_host(model_call("plp_model_covisibility_update_host", "G", neg_status=True), kf_lm, obs_offsets, obs_kf, kf_id, state, owners,
                                     kf_counts, lm_erased, outputs, out)


def model_covisibility_erase(state, erased, out=None):
    """Host build of graph_node::erase_all_connections for a set of key frames (csrc/covisibility.hpp, D21; no GPU needed): the arguments and the
    result of matcher.covisibility_erase."""
    return _covisibility_erase_host(model_call("plp_model_covisibility_erase_host", "F", neg_status=True), state, erased, out)


class covisibility_graph:
    """Mirror of data::graph_node (data/graph_node.h) for all F key frames of a map, over table rows: the connected maps, the ordered lists, the
    spanning parents.  mt: a matcher -- the tables live on its device as torch tensors and the calls are the _device entries -- or None = numpy
    tables and the host build.  After an OVERFLOW the touched rows are restored from the copy taken before the call, the cap that was outgrown
    is doubled and the call runs again."""

    def __init__(self, F, conn_cap=32, covis_cap=32, mt=None, device_index=0):
        self._mt, self.F = mt, int(F)
        st = covisibility_state(self.F, conn_cap, covis_cap)
        if mt is not None:
            import torch
            self._dev = torch.device("cuda", device_index)
            st = {k: torch.from_numpy(v).to(self._dev) for k, v in st.items()}
        self.state, self.last = st, None

    def _np(self, v):
        return v if isinstance(v, np.ndarray) else v.cpu().numpy()

    def _grow(self, conn, covis):
        """double the row length of the connected tables and / or of the ordered tables"""
        for k, (row, dt, fill) in COVISIBILITY_STATE.items():
            if row is None or not (conn if k.startswith("kf_conn") else covis):
                continue
            old = self.state[k]
            if isinstance(old, np.ndarray):
                new = np.full((self.F, max(2 * old.shape[1], 1)), fill, dt)
            else:
                new = old.new_full((self.F, max(2 * old.shape[1], 1)), fill)
            new[:, :old.shape[1]] = old
            self.state[k] = new

    def _run(self, names, call):
        """call(state) -> the outputs; the overflow protocol around it"""
        while True:
            keep = {k: (self.state[k].copy() if isinstance(self.state[k], np.ndarray) else self.state[k].clone()) for k in names}
            cc, vc = self.state["kf_conn"].shape[1], self.state["kf_covis"].shape[1]
            out = {k: self._np(v) for k, v in call(self.state).items()}
            if not (out["touched"] == 2).any():
                self.last = out
                return out
            rows = np.flatnonzero(out["touched"])
            n_conn, n_covis = self._np(self.state["kf_n_conn"]), self._np(self.state["kf_n_covis"])
            conn = bool((n_conn[rows] > cc).any())
            covis = bool((n_covis[rows] > vc).any())
            for k in names:                                  # the call was one transaction: every row it wrote goes back
                self.state[k][rows] = keep[k][rows]
            self._grow(conn or not covis, covis)

    def update_connections(self, rows, kf_lm, obs_offsets, obs_kf, kf_id, kf_counts=None, lm_erased=None):
        """update_connections() of the key frames `rows`, one after another in list order, over one map snapshot (numpy arrays, or torch tensors
        on the matcher's device).  Returns the statuses (G,); self.last holds every output."""
        owners = np.asarray(rows, np.int32).reshape(-1)
        if self._mt is None:
            call = lambda st: model_covisibility_update(kf_lm, obs_offsets, obs_kf, kf_id, st, owners, kf_counts, lm_erased)
        else:
            import torch
            dev = lambda v, dt: None if v is None else (v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dt)).to(self._dev))
            t = dict(kf_lm=dev(kf_lm, np.int32), kf_counts=dev(kf_counts, np.int32), obs_offsets=dev(obs_offsets, np.int32), obs_kf=dev(obs_kf, np.int32),
                     lm_erased=dev(lm_erased, np.uint8), kf_id=dev(np.asarray(kf_id).astype(np.uint32).view(np.int32) if not torch.is_tensor(kf_id) else kf_id, np.int32),
                     owners=dev(owners, np.int32))
            dims = dict(F=self.F, L=t["obs_offsets"].shape[0] - 1, T=t["obs_kf"].shape[0], cap=t["kf_lm"].shape[1] if self.F else 0, G=len(owners))

            def call(st):
                out = dict(status=torch.zeros(len(owners), dtype=torch.uint8, device=self._dev), nearest=torch.zeros(len(owners), dtype=torch.int32, device=self._dev),
                           max_weight=torch.zeros(len(owners), dtype=torch.int32, device=self._dev), touched=torch.zeros(self.F, dtype=torch.uint8, device=self._dev))
                self._mt.covisibility_update_device(dict(dims, conn_cap=st["kf_conn"].shape[1], covis_cap=st["kf_covis"].shape[1]), dict(t, **st), out)
                return out
        return self._run(tuple(COVISIBILITY_STATE), call)["status"]

    def erase_all_connections(self, rows_or_mask):
        """erase_all_connections() of the key frames named by a list of rows or by a mask of F bytes"""
        m = np.asarray(rows_or_mask)
        if not (m.dtype in (np.uint8, np.bool_) and m.shape == (self.F,)):
            rows, m = m.astype(np.int64).reshape(-1), np.zeros(self.F, np.uint8)
            m[rows] = 1
        m = m.astype(np.uint8)
        if self._mt is None:
            call = lambda st: model_covisibility_erase(st, m)
        else:
            import torch
            md = torch.from_numpy(m).to(self._dev)

            def call(st):
                out = dict(status=torch.zeros(self.F, dtype=torch.uint8, device=self._dev), touched=torch.zeros(self.F, dtype=torch.uint8, device=self._dev))
                self._mt.covisibility_erase_device(dict(F=self.F, conn_cap=st["kf_conn"].shape[1], covis_cap=st["kf_covis"].shape[1]), dict(st, erased=md), out)
                return out
        return self._run(COVISIBILITY_ERASE_STATE, call)["status"]

    def _ordered(self, row):
        n = int(self.state["kf_n_covis"][row])
        return self._np(self.state["kf_covis"][row, :n]), self._np(self.state["kf_covis_w"][row, :n])

    def get_covisibilities(self, row):
        return [int(v) for v in self._ordered(row)[0]]

    def get_top_n_covisibilities(self, row, n):
        return self.get_covisibilities(row)[:int(n)]

    def get_covisibilities_over_weight(self, row, weight):
        """the prefix whose weights are at least `weight` -- and the empty list when every entry qualifies, as the text returns (:262-266)"""
        rows, w = self._ordered(row)
        num = int((w >= int(weight)).sum())
        return [] if num == len(w) else [int(v) for v in rows[:num]]

    def get_connected_keyframes(self, row):
        n = int(self.state["kf_n_conn"][row])
        return {int(v) for v in self._np(self.state["kf_conn"][row, :n])}

    def get_weight(self, a, b):
        """the weight key frame a holds for key frame b, 0 when it holds none"""
        n = int(self.state["kf_n_conn"][a])
        rows, w = self._np(self.state["kf_conn"][a, :n]), self._np(self.state["kf_conn_w"][a, :n])
        at = np.flatnonzero(rows == int(b))
        return int(w[at[0]]) if len(at) else 0

    def get_spanning_parent(self, row):
        return int(self.state["kf_parent"][row])


class orb_extractor:
    """Mirror of feature::orb_extractor (src/PLPSLAM/feature/orb_extractor.h:38-176) over the C ABI."""

    DBG_BLURRED, DBG_CANDIDATES, DBG_SELECTED = 0, 1, 2

    def __init__(self, max_num_keypts=2000, scale_factor=1.2, num_levels=8, ini_fast_thr=20, min_fast_thr=7,
                 mask_rects=(), device=0):
        r = np.ascontiguousarray(np.asarray(mask_rects, np.float32).reshape(-1, 4))
        p = orb_params_c(max_num_keypts, scale_factor, num_levels, ini_fast_thr, min_fast_thr,
                         host_ptr(r), len(r))
        h = C.c_void_p()
        st = lib().plp_orb_create(C.byref(p), device, C.byref(h))
        if st == PLP_ERR_INVALID_ARG:
            raise ValueError(lib().plp_last_error().decode())   # the reference throws std::runtime_error here
        _check(st)
        self._h = h
        self.device = device

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().plp_orb_destroy(h)
            self._h = None

    # ---- getters / setters (orb_extractor.cc:162-233)
    def _get(self, i):
        v = C.c_double()
        _check(lib().plp_orb_get_param(self._h, i, C.byref(v)))
        return v.value

    def get_max_num_keypoints(self): return int(self._get(0))
    def set_max_num_keypoints(self, v): _check(lib().plp_orb_set_param(self._h, 0, float(v)))
    def get_scale_factor(self): return float(np.float32(self._get(1)))
    def set_scale_factor(self, v): _check(lib().plp_orb_set_param(self._h, 1, float(v)))
    def get_num_scale_levels(self): return int(self._get(2))
    def set_num_scale_levels(self, v): _check(lib().plp_orb_set_param(self._h, 2, float(v)))
    def get_initial_fast_threshold(self): return int(self._get(3))
    def set_initial_fast_threshold(self, v): _check(lib().plp_orb_set_param(self._h, 3, float(v)))
    def get_minimum_fast_threshold(self): return int(self._get(4))
    def set_minimum_fast_threshold(self, v): _check(lib().plp_orb_set_param(self._h, 4, float(v)))

    def _tables(self):
        n = self.get_num_scale_levels()
        f = [np.zeros(n, np.float32) for _ in range(4)]
        q = np.zeros(n, np.uint32)
        nl = C.c_int32()
        _check(lib().plp_orb_get_tables(self._h, C.byref(nl), *[_p(a) for a in f], _p(q)))
        return f, q

    def get_scale_factors(self): return self._tables()[0][0]
    def get_inv_scale_factors(self): return self._tables()[0][1]
    def get_level_sigma_sq(self): return self._tables()[0][2]
    def get_inv_level_sigma_sq(self): return self._tables()[0][3]
    def get_num_keypts_per_level(self): return self._tables()[1]

    # ---- extract (orb_extractor.cc:73-160): host image in, key points + descriptors out
    def extract(self, in_image, in_image_mask=None):
        img = _rows_u8(in_image)
        cap = 2 * self.get_max_num_keypoints() + 64
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int32(0)
        if img.size == 0:
            _check(lib().plp_orb_extract(self._h, None, 0, 0, 0, None, 0, _p(kps), _p(desc), cap, C.byref(n)))
            return kps[:0], desc[:0]
        mask = None if in_image_mask is None else _rows_u8(in_image_mask)
        _check(lib().plp_orb_extract(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0],
                                     _p(mask) if mask is not None else None,
                                     mask.strides[0] if mask is not None else 0, _p(kps), _p(desc), cap, C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    # ---- batched replay on device pointers (torch tensors own the HBM)
    def extract_batch(self, d_imgs, d_kps, d_desc, d_counts, d_mask=None, stream=None):
        """d_imgs: torch uint8 [B,H,W] on this device; outputs: d_kps uint8 [B,cap,28], d_desc uint8 [B,cap,32],
        d_counts int32 [B].  Asynchronous on `stream` (a torch.cuda.Stream; default = the current stream)."""
        import torch
        B, H, W = d_imgs.shape
        cap = d_kps.shape[1]
        assert d_imgs.is_cuda and d_imgs.dtype == torch.uint8 and d_imgs.stride(2) == 1
        st = (stream or torch.cuda.current_stream(d_imgs.device)).cuda_stream
        mptr, mstep, mfs = None, 0, 0
        if d_mask is not None:
            mptr, mstep = d_mask.data_ptr(), d_mask.stride(-2)
            mfs = d_mask.stride(0) if d_mask.dim() == 3 else 0
        _check(lib().plp_orb_extract_batch_device(self._h, d_imgs.data_ptr(), B, H, W, d_imgs.stride(1), d_imgs.stride(0),
                                                  mptr, mstep, mfs, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                                  d_counts.data_ptr(), st))

    def last_batch_status(self):
        _check(lib().plp_orb_last_batch_status(self._h))

    STAGES = ("l0_copy", "pyramid", "fast_cells", "blur7", "quadtree", "orient_rbrief", "batch_total")

    def set_profiling(self, on):
        _check(lib().plp_orb_set_profiling(self._h, int(bool(on))))

    def stage_times_ms(self):
        """(dict stage -> mean ms per batch, number of batches) accumulated since set_profiling(True)"""
        ms = np.zeros(7, np.float64)
        n = C.c_int64()
        _check(lib().plp_orb_get_stage_times(self._h, _p(ms), C.byref(n)))
        nb = max(n.value, 1)
        return {k: float(v) / nb for k, v in zip(self.STAGES, ms)}, n.value

    # ---- match::stereo(left pyramid, right pyramid, ...).compute (match/stereo.cc:45-150)
    def stereo_compute(self, right_extractor, keypts_left, keypts_right, descs_left, descs_right, focal_x_baseline, true_baseline):
        """self = left extractor; both extractors must have just extracted their image.  Returns (stereo_x_right, depths)."""
        kl = np.ascontiguousarray(keypts_left, KP_DTYPE); kr = np.ascontiguousarray(keypts_right, KP_DTYPE)
        dl = np.ascontiguousarray(descs_left, np.uint8); dr = np.ascontiguousarray(descs_right, np.uint8)
        xr = np.full(len(kl), -1, np.float32); dp = np.full(len(kl), -1, np.float32)
        _check(lib().plp_stereo_compute(self._h, right_extractor._h, _p(kl), len(kl), _p(kr), len(kr), _p(dl), _p(dr),
                                        float(focal_x_baseline), float(true_baseline), _p(xr), _p(dp)))
        return xr, dp

    # ---- image_pyramid_ (orb_extractor.h:101) and stage read-backs for parity tests
    def image_pyramid(self, level, frame=0):
        r, c = C.c_int32(), C.c_int32()
        _check(lib().plp_orb_pyramid_level_size(self._h, level, C.byref(r), C.byref(c)))
        a = np.zeros((r.value, c.value), np.uint8)
        _check(lib().plp_orb_pyramid_host(self._h, frame, level, _p(a), a.strides[0]))
        return a

    def debug_read(self, what, level, frame=0):
        r, c = C.c_int32(), C.c_int32()
        _check(lib().plp_orb_pyramid_level_size(self._h, level, C.byref(r), C.byref(c)))
        n = C.c_int64()
        if what == self.DBG_BLURRED:
            a = np.zeros((r.value, c.value), np.uint8)
            _check(lib().plp_orb_debug_read(self._h, what, frame, level, _p(a), a.nbytes, C.byref(n)))
            return a
        a = np.zeros((r.value * c.value // 4 + 16, 3), np.int32)
        _check(lib().plp_orb_debug_read(self._h, what, frame, level, _p(a), a.nbytes, C.byref(n)))
        return a[:n.value].copy()


# ------------------------------------------------------------------------------------------------
# Line front-end (feature::LineFeatureTracker of the reference)
# ------------------------------------------------------------------------------------------------
class LineFeatureTracker:
    """Mirror of feature::LineFeatureTracker (src/PLPSLAM/feature/line_extractor.h:61-104) over the C ABI."""

    DBG_SCALED, DBG_ORDER, DBG_RAW, DBG_ALL_KL, DBG_ALL_LBD, DBG_SOBEL_DX, DBG_SOBEL_DY, DBG_GROW_STATS = range(8)

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().plp_line_create(device, C.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().plp_line_destroy(h)
            self._h = None

    def extract_LSD_LBD(self, img):
        """returns (frame_keylsd, frame_lbd_descr, keyline_functions) like line_extractor.cc:88-160"""
        img = _rows_u8(img)
        kl = np.zeros(LINE_CAP, KL_DTYPE)
        lbd = np.zeros((LINE_CAP, 32), np.uint8)
        fn = np.zeros((LINE_CAP, 3), np.float64)
        n = C.c_int32(0)
        _check(lib().plp_line_extract(self._h, _p(img), img.shape[0], img.shape[1], img.strides[0], _p(kl), _p(lbd), _p(fn), LINE_CAP, C.byref(n)))
        return kl[:n.value].copy(), lbd[:n.value].copy(), fn[:n.value].copy()

    def set_seed_order(self, order):
        """SEED_ORDER_LIBSTDCXX: the seed order of a reference built with GCC's library, SEED_ORDER_STABLE: row-major inside a bin (plp_line_set_seed_order)"""
        _check(lib().plp_line_set_seed_order(self._h, int(order)))

    def trim(self):
        """give back the device memory the current settings do not need (plp_line_trim: the exact order's buffers under SEED_ORDER_STABLE, the several-waves heap)"""
        _check(lib().plp_line_trim(self._h))

    def set_grow_waves(self, waves):
        """0 = automatic, 1 = one wave per frame in LSD region growing, 2..8 = that many waves per frame (plp_line_set_grow_waves)"""
        _check(lib().plp_line_set_grow_waves(self._h, int(waves)))

    def extract_batch(self, d_imgs, d_kl, d_lbd, d_fn, d_counts, stream=None):
        """d_imgs torch uint8 [B,H,W]; d_kl uint8 [B,cap,68]; d_lbd uint8 [B,cap,32]; d_fn float64 [B,cap,3]; d_counts int32 [B]"""
        import torch
        B, H, W = d_imgs.shape
        st = (stream or torch.cuda.current_stream(d_imgs.device)).cuda_stream
        _check(lib().plp_line_extract_batch_device(self._h, d_imgs.data_ptr(), B, H, W, d_imgs.stride(1), d_imgs.stride(0), d_kl.data_ptr(),
                                                   d_lbd.data_ptr(), d_fn.data_ptr(), d_kl.shape[1], d_counts.data_ptr(), st))

    def last_batch_status(self):
        _check(lib().plp_line_last_batch_status(self._h))

    STAGES = ("lsd_blur11_resize", "lsd_gradient_bins", "lsd_order", "lsd_grow", "keylines", "lbd_blur5_sobel", "lbd", "line_finalize", "batch_total")

    def set_profiling(self, on):
        _check(lib().plp_line_set_profiling(self._h, int(bool(on))))

    def stage_times_ms(self):
        ms = np.zeros(9, np.float64)
        n = C.c_int64()
        _check(lib().plp_line_get_stage_times(self._h, _p(ms), C.byref(n)))
        nb = max(n.value, 1)
        return {k: float(v) / nb for k, v in zip(self.STAGES, ms)}, n.value

    def grow_profile(self):
        v = np.zeros(12, np.int64)
        _check(lib().plp_line_debug_grow_profile(self._h, _p(v)))
        d = dict(zip(("cycles_total", "cycles_grow", "cycles_rect", "cycles_refine", "regions", "pixels"), v[:6].tolist()))
        d["more"] = v[6:].tolist()
        return d

    def debug_read(self, what, frame=0):
        r, c = C.c_int32(), C.c_int32()
        _check(lib().plp_line_scaled_size(self._h, C.byref(r), C.byref(c)))
        n = C.c_int64()
        if what == self.DBG_SCALED:
            a = np.zeros((r.value, c.value), np.uint8)
        elif what == self.DBG_ORDER:
            a = np.zeros((r.value - 1) * (c.value - 1), np.int32)
        elif what == self.DBG_RAW:
            a = np.zeros((LINE_CAP, 4), np.float32)
        elif what == self.DBG_ALL_KL:
            a = np.zeros(LINE_CAP, KL_DTYPE)
        elif what == self.DBG_ALL_LBD:
            a = np.zeros((LINE_CAP, 32), np.uint8)
        elif what == self.DBG_GROW_STATS:
            a = np.zeros(4, np.int32)
        else:
            a = np.zeros(4 * r.value * c.value + 4 * (r.value + c.value) + 8, np.int16)
        _check(lib().plp_line_debug_read(self._h, what, frame, _p(a), a.nbytes, C.byref(n)))
        if what in (self.DBG_RAW, self.DBG_ALL_KL, self.DBG_ALL_LBD, self.DBG_ORDER):
            return a[:n.value].copy()
        if what in (self.DBG_SOBEL_DX, self.DBG_SOBEL_DY):
            return a[:n.value].copy()
        return a


# ------------------------------------------------------------------------------------------------
# Hamming matchers, array form (match::projection / match::robust of the reference)
# ------------------------------------------------------------------------------------------------
class camera_model(camera_model_c):
    """Mirror of the camera the reference's config builds from the yaml's Camera.* keys (config.cc:62-72 switches on Camera.model):
    camera::perspective (perspective.cc:59-75), camera::fisheye (fisheye.cc:59-75) or camera::equirectangular (equirectangular.cc:45-50).
    The object IS the plp_camera_model struct (ctypes.byref(cam) goes to plp_post_extract_model_*); img_bounds is camera::base
    img_bounds_ (min_x, max_x, min_y, max_y as float32, camera/base.h:68-82) and grid() the matcher grid the constructors derive from it."""

    NUM_GRID_COLS, NUM_GRID_ROWS = 64, 48      # camera::base defaults (camera/base.h:91)

    def __init__(self, yaml_node, device=0):
        super().__init__()
        name = yaml_node["Camera.model"]
        if name not in CAMERA_MODEL_NAMES:
            raise PlpError(PLP_ERR_INVALID_ARG, f"Invalid camera model: {name}")
        self.model = CAMERA_MODEL_NAMES[name]
        self.cols, self.rows = int(yaml_node["Camera.cols"]), int(yaml_node["Camera.rows"])
        if self.model != CAMERA_EQUIRECTANGULAR:
            dist = ("k1", "k2", "p1", "p2", "k3") if self.model == CAMERA_PERSPECTIVE else ("k1", "k2", "k3", "k4")
            for k in ("fx", "fy", "cx", "cy") + dist:
                setattr(self, k, float(yaml_node[f"Camera.{k}"]))
            self.focal_x_baseline = float(yaml_node.get("Camera.focal_x_baseline", 0.0))
        self.device = device
        self._bounds = None

    @property
    def img_bounds(self):
        """(min_x, max_x, min_y, max_y) float32: compute_image_bounds() of the model (the distorted corners go through the GPU's undistortion)"""
        if self._bounds is None:
            self._bounds = self._compute_image_bounds()
        return self._bounds

    def _undistort(self, pts):
        k = np.zeros(len(pts), KP_DTYPE)
        k["x"] = [np.float32(x) for x, _ in pts]; k["y"] = [np.float32(y) for _, y in pts]; k["size"] = 1.0   # cv::KeyPoint(x, y, 1.0): float x, y
        u = matcher(device=self.device).post_extract(self, k)["undist_keypts"]
        return [(np.float32(a), np.float32(b)) for a, b in zip(u["x"], u["y"])]

    def _compute_image_bounds(self):
        f32 = np.float32
        cols, rows = f32(self.cols), f32(self.rows)            # unsigned int -> float
        whole = np.array([0.0, cols, 0.0, rows], np.float32)
        if self.model == CAMERA_EQUIRECTANGULAR:                # equirectangular.cc:62-67
            return whole
        lo = lambda a, b: b if b < a else a                     # std::min / std::max
        hi = lambda a, b: b if a < b else a
        if self.model == CAMERA_PERSPECTIVE:                    # perspective.cc:100-128
            if self.k1 == 0 and self.k2 == 0 and self.p1 == 0 and self.p2 == 0 and self.k3 == 0:
                return whole
            c = self._undistort([(0.0, 0.0), (cols, 0.0), (0.0, rows), (cols, rows)])
            return np.array([lo(c[0][0], c[2][0]), hi(c[1][0], c[3][0]), lo(c[0][1], c[1][1]), hi(c[2][1], c[3][1])], np.float32)
        # fisheye.cc:98-168
        if self.k1 == 0 and self.k2 == 0 and self.k3 == 0 and self.k4 == 0:
            return whole
        pwx, pwy = (0.0 - self.cx) / self.fx, (0.0 - self.cy) / self.fy
        if math.sqrt(pwx * pwx + pwy * pwy) > math.pi / 2:       # super wide: the four corners are out of view (edge midpoints, 5 degree limit)
            c = self._undistort([(self.cx, 0.0), (cols, self.cy), (0.0, self.cy), (self.cx, rows)])
            dist_thr_x = f32(self.fx / math.tan(5.0 * math.pi / 180.0))
            dist_thr_y = f32(self.fy / math.tan(5.0 * math.pi / 180.0))
            min_x_thr, max_x_thr = f32(-float(dist_thr_x) + self.cx), f32(float(dist_thr_x) + self.cx)
            min_y_thr, max_y_thr = f32(-float(dist_thr_y) + self.cy), f32(float(dist_thr_y) + self.cy)
            umin_x, umax_x, umin_y, umax_y = c[2][0], c[1][0], c[0][1], c[3][1]
            return np.array([min_x_thr if (umin_x < min_x_thr or float(umin_x) > self.cx) else umin_x,
                             max_x_thr if (umax_x > max_x_thr or float(umax_x) < self.cx) else umax_x,
                             min_y_thr if (umin_y < min_y_thr or float(umin_y) > self.cy) else umin_y,
                             max_y_thr if (umax_y > max_y_thr or float(umax_y) < self.cy) else umax_y], np.float32)
        c = self._undistort([(0.0, 0.0), (cols, 0.0), (0.0, rows), (cols, rows)])
        return np.array([lo(c[0][0], c[2][0]), hi(c[1][0], c[3][0]), lo(c[0][1], c[1][1]), hi(c[2][1], c[3][1])], np.float32)

    def grid(self):
        """camera::base grid: inv_cell_width = (double)num_grid_cols / (float)(max_x - min_x) (fisheye.cc:55-56 and the other two constructors)"""
        b = self.img_bounds
        inv_w = np.float64(self.NUM_GRID_COLS) / np.float64(np.float32(b[1] - b[0]))
        inv_h = np.float64(self.NUM_GRID_ROWS) / np.float64(np.float32(b[3] - b[2]))
        return match_grid_c(float(b[0]), float(b[2]), float(inv_w), float(inv_h), self.NUM_GRID_COLS, self.NUM_GRID_ROWS)


def frame_pose(rot_cw, trans_cw):
    """One problem's pose row of plp_observe_args (15 doubles): rot_cw_ row-major, trans_cw_ and cam_center_ = -rot_cw_^T trans_cw_ formed as
    frame::update_pose_params does (frame.cc:745-751; each coefficient a left-to-right sum of the negated column times trans_cw_)."""
    R = [[float(v) for v in row] for row in np.asarray(rot_cw, np.float64).reshape(3, 3)]
    t = [float(v) for v in np.asarray(trans_cw, np.float64).reshape(3)]
    cc = [((-R[0][i]) * t[0] + (-R[1][i]) * t[1]) + (-R[2][i]) * t[2] for i in range(3)]
    return np.array(R[0] + R[1] + R[2] + t + cc, np.float64)


def _camera_args(cls, camera, img_bounds, B, m_cap, fields, ptrs):
    """an args struct that begins with the camera and the image bounds (the camera's own unless given)"""
    a = _struct(cls, dict(fields, B=int(B), m_cap=int(m_cap)), ptrs)
    a.camera = camera_model_c.from_buffer_copy(camera)
    a.img_bounds[:] = [float(np.float32(v)) for v in (camera.img_bounds if img_bounds is None else img_bounds)]
    return a


def _observe_args(camera, img_bounds, ray_cos_thr, log_scale_factor, num_levels, B, m_cap, ptrs):
    return _camera_args(observe_args_c, camera, img_bounds, B, m_cap, dict(
        ray_cos_thr=float(ray_cos_thr), log_scale_factor=float(np.float32(log_scale_factor)), num_levels=int(num_levels)), ptrs)


def _last_frame_args(camera, img_bounds, setup_type, true_baseline, B, m_cap, ptrs):
    return _camera_args(last_frame_args_c, camera, img_bounds, B, m_cap, dict(setup_type=int(setup_type), true_baseline=float(true_baseline)), ptrs)


def _project_args(camera, img_bounds, log_scale_factor, num_levels, B, m_cap, shared_landmarks, dist_mode, ray_test, line_dist_mode, ptrs):
    return _camera_args(project_args_c, camera, img_bounds, B, m_cap, dict(
        log_scale_factor=float(np.float32(log_scale_factor)), num_levels=int(num_levels), shared_landmarks=int(bool(shared_landmarks)),
        dist_mode=int(dist_mode), ray_test=int(bool(ray_test)), line_dist_mode=int(line_dist_mode)), ptrs)


def _mat3(m):
    return [[float(v) for v in row] for row in np.asarray(m, np.float64).reshape(3, 3)]


def _vec3(v):
    return [float(t) for t in np.asarray(v, np.float64).reshape(3)]


def _mul33(A, Bm):
    """Eigen's 3 x 3 product: every coefficient summed left to right over k"""
    return [[(A[i][0] * Bm[0][j] + A[i][1] * Bm[1][j]) + A[i][2] * Bm[2][j] for j in range(3)] for i in range(3)]


def _mul3v(A, v):
    return [(A[i][0] * v[0] + A[i][1] * v[1]) + A[i][2] * v[2] for i in range(3)]


def sim3_pose(Sim3_cw):
    """The pose row of plp_project_args for a Sim3 (fuse.cc:46-50, projection.cc:787-791): s_cw = sqrt of the left-to-right dot of row 0 of
    the scaled rotation, rot_cw = s_rot_cw / s_cw and trans_cw = Sim3_cw.block<3, 1>(0, 3) / s_cw coefficient by coefficient, cam_center =
    -rot_cw^T trans_cw formed as frame_pose forms it."""
    S = [[float(v) for v in row] for row in np.asarray(Sim3_cw, np.float64).reshape(4, 4)]
    s_cw = math.sqrt((S[0][0] * S[0][0] + S[0][1] * S[0][1]) + S[0][2] * S[0][2])
    rot = [[S[i][j] / s_cw for j in range(3)] for i in range(3)]
    trans = [S[i][3] / s_cw for i in range(3)]
    return frame_pose(rot, trans)


def mutual_poses(s_12, rot_12, trans_12, rot_1w, trans_1w, rot_2w, trans_2w):
    """The two pose rows of projection::match_keyframes_mutually (projection.cc:906-908, 941-942, 1035-1036), (2, 15): row 0 = s_rot_21w,
    trans_21w (landmarks of key frame 1 into key frame 2), row 1 = s_rot_12w, trans_12w (landmarks of key frame 2 into key frame 1).  s_12 is
    the reference's float; s_rot_12 = s_12 * rot_12, s_rot_21 = (1.0 / s_12) * rot_12^T, trans_21 = -s_rot_21 * trans_12; every product is
    summed left to right over k.  Entries 12-14 (cam_center) are 0: both passes measure the distance in the camera frame
    (PROJECT_DIST_CAMERA)."""
    s = float(np.float32(s_12))
    R12, R1w, R2w = _mat3(rot_12), _mat3(rot_1w), _mat3(rot_2w)
    t12, t1w, t2w = _vec3(trans_12), _vec3(trans_1w), _vec3(trans_2w)
    inv = 1.0 / s
    s_rot_12 = [[s * R12[i][j] for j in range(3)] for i in range(3)]
    s_rot_21 = [[inv * R12[j][i] for j in range(3)] for i in range(3)]
    trans_21 = _mul3v([[-v for v in row] for row in s_rot_21], t12)
    s_rot_21w = _mul33(s_rot_21, R1w)
    trans_21w = [a + b for a, b in zip(_mul3v(s_rot_21, t1w), trans_21)]
    s_rot_12w = _mul33(s_rot_12, R2w)
    trans_12w = [a + b for a, b in zip(_mul3v(s_rot_12, t2w), t12)]
    flat = lambda M: M[0] + M[1] + M[2]
    return np.array([flat(s_rot_21w) + trans_21w + [0.0] * 3, flat(s_rot_12w) + trans_12w + [0.0] * 3], np.float64)


def make_grid(cols_px, rows_px, grid_cols=64, grid_rows=48, min_x=0.0, min_y=0.0):
    """camera::base grid for an undistorted image of cols_px x rows_px (camera/base.h:91, perspective.cc ctor)."""
    inv_w = np.float64(grid_cols) / np.float64(np.float32(cols_px) - np.float32(min_x))   # perspective.cc:55-56
    inv_h = np.float64(grid_rows) / np.float64(np.float32(rows_px) - np.float32(min_y))
    return match_grid_c(min_x, min_y, float(inv_w), float(inv_h), grid_cols, grid_rows)


MATCH_PLAN_TOPK = {0: None, 1: "cells", 2: "lds", 3: "lanes", 4: "topk", 5: "fuse"}
MATCH_PLAN_FAMILY = {0: "any", 1: "line", 2: "group", 3: "point", 4: "grid"}
MATCH_PLAN_RESOLVE = {0: None, 1: "sorted", 2: "generic"}


def match_plan(mode, B, n_cap, m_cap, grid=None, t_x_right=False, t_count_hint=0):
    """The kernels plp_match_host / plp_match_device run for a call of this shape (plp_match_debug_plan; no device needed):
    (top-k kernel, family, queries per workgroup, resolve kernel), e.g. ("cells", "grid", 32, "sorted"); (None, "any", 0, None) for an empty side.
    t_x_right: whether the call passes t_x_right (it sizes the LDS staging of the windowed modes)."""
    a = match_args_c()
    a.mode, a.B, a.n_cap, a.m_cap, a.t_count_hint = mode, B, n_cap, m_cap, int(t_count_hint)
    keep = np.zeros(1, np.float32)
    a.t_x_right = keep.ctypes.data if t_x_right else None
    if grid is not None:
        a.grid = grid
    out = np.zeros(4, np.int32)
    _check(lib().plp_match_debug_plan(C.byref(a), _p(out)))
    return MATCH_PLAN_TOPK[int(out[0])], MATCH_PLAN_FAMILY[int(out[1])], int(out[2]), MATCH_PLAN_RESOLVE[int(out[3])]


class matcher(line_update_entries):
    """Array-form mirror of match::projection / match::robust (value-constructed with (lowe_ratio, check_orientation)
    at every call site of the reference, match/base.h:94-110)."""

    def __init__(self, lowe_ratio=0.6, check_orientation=True, device=0):
        h = C.c_void_p()
        _check(lib().plp_matcher_create(device, C.byref(h)))
        self._h = h
        self.device = device
        self.lowe_ratio = lowe_ratio
        self.check_orientation = check_orientation
        self._keep = []

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().plp_matcher_destroy(h)
            self._h = None

    def _host(self, symbol):
        """call(args struct) for the host-pointer entry `symbol` of this context"""
        return lambda a: _check(getattr(lib(), symbol)(self._h, C.byref(a)))

    def _device(self, symbol, a, stream):
        """the device-pointer entry `symbol` of this context on the stream (int handle, torch stream or None = torch's current one); asynchronous"""
        _check(getattr(lib(), symbol)(self._h, C.byref(a), stream_handle(stream)))

    def _args(self, mode, B, n_cap, m_cap, fields, margin, direction, scale_factors, grid, out_match, out_num, ptr):
        a = match_args_c()
        a.mode, a.B, a.n_cap, a.m_cap = mode, B, n_cap, m_cap
        for k, v in fields.items():
            if k in ("is_rgbd", "num_levels_lsd", "hamm_dist_thr", "level_window", "flags", "q_desc_stride", "t_count_hint"):
                setattr(a, k, int(v))
            elif k == "inv_level_sigma_sq":
                arr = np.ascontiguousarray(v, np.float32)
                self._keep2 = arr
                a.inv_level_sigma_sq = arr.ctypes.data
            else:
                setattr(a, k, ptr(v) if v is not None else None)
        a.margin, a.lowe_ratio = margin, self.lowe_ratio
        a.direction, a.check_orientation = direction, int(self.check_orientation)
        if scale_factors is not None:
            sf = np.ascontiguousarray(scale_factors, np.float32)
            self._keep = [sf]
            a.num_levels, a.scale_factors = len(sf), sf.ctypes.data
        if grid is not None:
            a.grid = grid
        a.out_match, a.out_num = ptr(out_match), ptr(out_num)
        return a

    def match_host(self, mode, n_cap, m_cap, fields, margin=0.0, direction=0, scale_factors=None, grid=None, B=1, directions=None,
                   out_match=None, out_num=None, out_query_best=None):
        """fields: dict of numpy arrays named like plp_match_args members.  Returns (out_match [B,n_cap], out_num [B]).
        directions: B int32 (plp_match_args.directions: LAST_FRAME[_LINE] per problem), None = `direction` for every problem.
        out_match / out_num / out_query_best: C-contiguous int32 arrays [B, n_cap] / [B] / [B, m_cap] the call writes into (and returns);
        the slots beyond a problem's t_counts / q_counts keep what they hold.  None: fresh arrays."""
        fields = {k: (v if (v is None or np.isscalar(v)) else np.ascontiguousarray(v)) for k, v in fields.items()}
        if directions is not None:
            fields["directions"] = np.ascontiguousarray(directions, np.int32).reshape(B)

        def given(a, shape):
            assert isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == shape and a.flags.c_contiguous, (shape, a)
            return a
        out_match = np.zeros((B, n_cap), np.int32) if out_match is None else given(out_match, (B, n_cap))
        out_num = np.zeros(B, np.int32) if out_num is None else given(out_num, (B,))
        a = self._args(mode, B, n_cap, m_cap, fields, margin, direction, scale_factors, grid, out_match, out_num, lambda v: v.ctypes.data)
        if mode in (MODE_FUSE, MODE_FUSE_LINE):
            out_q = np.full((B, m_cap), -1, np.int32) if out_query_best is None else given(out_query_best, (B, m_cap))
            a.out_query_best = out_q.ctypes.data
            _check(lib().plp_match_host(self._h, C.byref(a)))
            return out_q
        _check(lib().plp_match_host(self._h, C.byref(a)))
        return out_match, out_num

    def match_device(self, mode, n_cap, m_cap, fields, out_match, out_num, margin=0.0, direction=0, scale_factors=None, grid=None,
                     B=1, stream=None, directions=None):
        """fields / outputs: torch tensors on the matcher's device.  Asynchronous.  directions: B int32 on the device
        (e.g. out_direction of project_last_frame[_lines]_device), None = `direction` for every problem."""
        import torch
        st = (stream or torch.cuda.current_stream(out_match.device)).cuda_stream
        if directions is not None:
            fields = {**fields, "directions": directions}
        a = self._args(mode, B, n_cap, m_cap, fields, margin, direction, scale_factors, grid, out_match, out_num, lambda v: v.data_ptr())
        _check(lib().plp_match_device(self._h, C.byref(a), st))

    def match_in_consistent_area(self, kps_1, desc_1, kps_2, desc_2, prev_matched_pts, margin, grid):
        """area::match_in_consistent_area: returns (matched_indices_2_in_frm_1, updated prev_matched_pts, num_matches)"""
        k1 = np.ascontiguousarray(kps_1, KP_DTYPE); k2 = np.ascontiguousarray(kps_2, KP_DTYPE)
        d1 = np.ascontiguousarray(desc_1, np.uint8); d2 = np.ascontiguousarray(desc_2, np.uint8)
        pp = np.ascontiguousarray(prev_matched_pts, np.float32).copy()
        out = np.full(max(len(k1), 1), -1, np.int32)
        num = C.c_int32(0)
        _check(lib().plp_match_area_host(self._h, _p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), C.byref(grid), _p(pp), int(margin),
                                         float(self.lowe_ratio), int(self.check_orientation), _p(out), C.byref(num)))
        return out[:len(k1)].copy(), pp, num.value

    def landmark_descriptors(self, descs, offsets):
        """landmark::compute_descriptor for L landmarks: descs [total, 32] u8, offsets [L + 1] -> best row per landmark (-1: none)"""
        d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32); o = np.ascontiguousarray(offsets, np.int32)
        out = np.zeros(max(len(o) - 1, 1), np.int32)
        _check(lib().plp_landmark_descriptor_host(self._h, _p(d) if len(d) else None, _p(o), len(o) - 1, _p(out)))
        return out[:len(o) - 1].copy()

    def post_extract(self, camera, keypts, depth=None, keylines=None, kl_depths=None, kl_x_right=None):
        """undistort_keypoints + convert_keypoints_to_bearings (+ compute_stereo_from_depth when a depth image is given).
        camera: a camera_c (perspective, plp_post_extract_host) or a camera_model / camera_model_c (any model, plp_post_extract_model_host).
        Returns dict(undist_keypts, bearings[, stereo_x_right, depths][, kl_depths, kl_x_right])."""
        k = np.ascontiguousarray(keypts, KP_DTYPE)
        n = len(k)
        und = np.zeros(max(n, 1), KP_DTYPE); bear = np.zeros((max(n, 1), 3), np.float64)
        xr = np.zeros(max(n, 1), np.float32); dep = np.zeros(max(n, 1), np.float32)
        d = None if depth is None else (depth if (isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.ndim == 2 and depth.size and depth.strides[1] == 4
                                                and depth.strides[0] >= 4 * depth.shape[1]) else np.ascontiguousarray(depth, np.float32))   # (a view with a row step goes as it is)
        kl = np.ascontiguousarray(keylines, KL_DTYPE) if keylines is not None else None
        nl = len(kl) if kl is not None else 0
        kd = np.ascontiguousarray(kl_depths, np.float32).copy() if kl is not None else None
        kx = np.ascontiguousarray(kl_x_right, np.float32).copy() if kl is not None else None
        entry = lib().plp_post_extract_model_host if isinstance(camera, camera_model_c) else lib().plp_post_extract_host
        _check(entry(self._h, C.byref(camera), _p(k) if n else None, n, _p(d) if d is not None else None,
                                           d.shape[0] if d is not None else 0, d.shape[1] if d is not None else 0, d.strides[0] if d is not None else 0,
                                           _p(und), _p(bear), _p(xr) if d is not None else None, _p(dep) if d is not None else None,
                                           _p(kl) if nl else None, nl, _p(kd) if nl else None, _p(kx) if nl else None))
        out = dict(undist_keypts=und[:n].copy(), bearings=bear[:n].copy())
        if d is not None:
            out.update(stereo_x_right=xr[:n].copy(), depths=dep[:n].copy())
        if kl is not None:
            out.update(kl_depths=kd, kl_x_right=kx)
        return out

    # ---- local-landmark visibility: the queries of match_frame_and_landmarks[_line] (tracking_module.cc:908-1064, plp_observe_landmark[_line]s_*)
    def _observe_host(self, lines, camera, pose, pos_w, obs_mean_normal, min_valid_dist, max_valid_dist, skip, counts, ray_cos_thr, log_scale_factor,
                      num_levels, img_bounds):
        pose = np.ascontiguousarray(pose, np.float64)
        single = pose.ndim == 1
        pose = pose.reshape(-1, 15)
        B = len(pose)
        w = 6 if lines else 3
        pw = np.ascontiguousarray(pos_w, np.float64).reshape(B, -1, w)
        M = pw.shape[1]
        arr = lambda v, dt, *shape: None if v is None else np.ascontiguousarray(v, dt).reshape(B, M, *shape)
        nm = None if lines else arr(obs_mean_normal, np.float64, 3)
        mn, mx, sk = arr(min_valid_dist, np.float32), arr(max_valid_dist, np.float32), arr(skip, np.uint8)
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(B)
        out = dict(reproj=np.zeros((B, M, 2), np.float32), level=np.zeros((B, M), np.int32), valid=np.zeros((B, M), np.uint8), num_valid=np.zeros(B, np.int32))
        if lines:
            out["reproj_ep"] = np.zeros((B, M, 2), np.float32)
        else:
            out["x_right"] = np.zeros((B, M), np.float32)
        a = _observe_args(camera, img_bounds, ray_cos_thr, log_scale_factor, num_levels, B, M, host_ptrs(
            empty_null=False,   # these entries check their pointers before m_cap / cap
            pose=pose, counts=cn, pos_w=pw, obs_mean_normal=nm, min_valid_dist=mn, max_valid_dist=mx, skip=sk,
            out_reproj=out["reproj"], out_reproj2=out.get("reproj_ep"), out_x_right=out.get("x_right"), out_level=out["level"],
            out_valid=out["valid"], out_num_valid=out["num_valid"]))
        self._host("plp_observe_landmark_lines_host" if lines else "plp_observe_landmarks_host")(a)
        if lines:
            out["reproj_sp"] = out.pop("reproj")
        return {k: v[0] for k, v in out.items()} if single else out

    def observe_landmarks(self, camera, pose, pos_w, obs_mean_normal=None, min_valid_dist=None, max_valid_dist=None, skip=None, counts=None,
                          ray_cos_thr=0.5, log_scale_factor=None, num_levels=8, img_bounds=None):
        """frame::can_observe over a frame's local landmarks (tracking_module.cc:929-965).  camera: camera_model (img_bounds from it unless given);
        pose: frame_pose(...) of one frame (15,) or of B frames (B, 15); pos_w (m, 3) / (B, m, 3); obs_mean_normal None = reprojection only.
        log_scale_factor defaults to frame::log_scale_factor_ of the scale factor 1.2f (logf as D5 defines it).  Returns dict(reproj, x_right, level, valid,
        num_valid); the library does not write reproj / x_right / level of invalid slots, so they hold 0."""
        lsf = np.float32(math.log(np.float32(1.2))) if log_scale_factor is None else log_scale_factor
        return self._observe_host(False, camera, pose, pos_w, obs_mean_normal, min_valid_dist, max_valid_dist, skip, counts, ray_cos_thr, lsf,
                                  num_levels, img_bounds)

    def observe_landmark_lines(self, camera, pose, pos_w, min_valid_dist, max_valid_dist, skip=None, counts=None, log_scale_factor=None,
                               num_levels=2, img_bounds=None):
        """frame::can_observe_line over a frame's local line landmarks (tracking_module.cc:1004-1045).  pos_w (m, 6) / (B, m, 6): start point,
        end point; log_scale_factor / num_levels = _log_scale_factor_lsd / _num_scale_levels_lsd (default: scale factor 2, 2 levels).
        Returns dict(reproj_sp, reproj_ep, level, valid, num_valid); reproj_sp / reproj_ep of every slot are the reference's temporaries after it
        (DESIGN.md section 5, D5 item 5)."""
        lsf = np.float32(math.log(np.float32(2.0))) if log_scale_factor is None else log_scale_factor
        return self._observe_host(True, camera, pose, pos_w, None, min_valid_dist, max_valid_dist, skip, counts, 0.0, lsf, num_levels, img_bounds)

    def _observe_device(self, lines, camera, B, m_cap, pose, pos_w, out_reproj, out_valid, obs_mean_normal, min_valid_dist, max_valid_dist, skip,
                        counts, out_reproj2, out_x_right, out_level, out_num_valid, ray_cos_thr, log_scale_factor, num_levels, img_bounds, stream):
        a = _observe_args(camera, img_bounds, ray_cos_thr, log_scale_factor, num_levels, B, m_cap, dev_ptrs(
            pose=pose, counts=counts, pos_w=pos_w, obs_mean_normal=obs_mean_normal, min_valid_dist=min_valid_dist, max_valid_dist=max_valid_dist, skip=skip,
            out_reproj=out_reproj, out_reproj2=out_reproj2, out_x_right=out_x_right, out_level=out_level, out_valid=out_valid, out_num_valid=out_num_valid))
        self._device("plp_observe_landmark_lines_device" if lines else "plp_observe_landmarks_device", a, stream)

    def observe_landmarks_device(self, camera, B, m_cap, pose, pos_w, out_reproj, out_valid, obs_mean_normal=None, min_valid_dist=None,
                                 max_valid_dist=None, skip=None, counts=None, out_x_right=None, out_level=None, out_num_valid=None, ray_cos_thr=0.5,
                                 log_scale_factor=None, num_levels=8, img_bounds=None, stream=None):
        """plp_observe_landmarks_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        lsf = np.float32(math.log(np.float32(1.2))) if log_scale_factor is None else log_scale_factor
        self._observe_device(False, camera, B, m_cap, pose, pos_w, out_reproj, out_valid, obs_mean_normal, min_valid_dist, max_valid_dist, skip,
                             counts, None, out_x_right, out_level, out_num_valid, ray_cos_thr, lsf, num_levels, img_bounds, stream)

    def observe_landmark_lines_device(self, camera, B, m_cap, pose, pos_w, min_valid_dist, max_valid_dist, out_reproj_sp, out_reproj_ep, out_level,
                                      out_valid, skip=None, counts=None, out_num_valid=None, log_scale_factor=None, num_levels=2, img_bounds=None,
                                      stream=None):
        """plp_observe_landmark_lines_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        lsf = np.float32(math.log(np.float32(2.0))) if log_scale_factor is None else log_scale_factor
        self._observe_device(True, camera, B, m_cap, pose, pos_w, out_reproj_sp, out_valid, None, min_valid_dist, max_valid_dist, skip, counts,
                             out_reproj_ep, None, out_level, out_num_valid, 0.0, lsf, num_levels, img_bounds, stream)

    # ---- last-frame queries: the loops in front of match_current_and_last_frames[_line] (projection.cc:214-527, plp_project_last_frame[_lines]_*)
    def _last_frame_host(self, lines, camera, pose_curr, pose_last, pos_w, feats, skip, counts, setup_type, true_baseline, img_bounds, out):
        pc = np.ascontiguousarray(pose_curr, np.float64)
        single = pc.ndim == 1
        pc = pc.reshape(-1, 15)
        B = len(pc)
        pl = np.ascontiguousarray(pose_last, np.float64).reshape(B, 15)
        w = 6 if lines else 3
        pw = np.ascontiguousarray(pos_w, np.float64).reshape(B, -1, w)
        M = pw.shape[1]
        ft = np.ascontiguousarray(feats, KL_DTYPE if lines else KP_DTYPE).reshape(B, M)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(B, M)
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(B)
        specs = (("reproj", (B, M, 2), np.float32), ("x_right", (B, M), np.float32), ("level", (B, M), np.int32), ("valid", (B, M), np.uint8),
                 ("direction", (B,), np.int32), ("num_valid", (B,), np.int32))
        specs += (("reproj_ep", (B, M, 2), np.float32), ("x_right_ep", (B, M), np.float32)) if lines else (("angle", (B, M), np.float32),)
        o = out_arrays(specs, out)
        a = _last_frame_args(camera, img_bounds, setup_type, true_baseline, B, M, host_ptrs(
            empty_null=False,   # these entries check their pointers before m_cap / cap
            counts=cn, pose_curr=pc, pose_last=pl, pos_w=pw, skip=sk, keypts=None if lines else ft, keylines=ft if lines else None,
            out_reproj=o["reproj"], out_reproj2=o.get("reproj_ep"), out_x_right=o["x_right"], out_x_right2=o.get("x_right_ep"),
            out_level=o["level"], out_angle=o.get("angle"), out_valid=o["valid"], out_direction=o["direction"], out_num_valid=o["num_valid"]))
        self._host("plp_project_last_frame_lines_host" if lines else "plp_project_last_frame_host")(a)
        if lines:
            o["reproj_sp"], o["x_right_sp"] = o.pop("reproj"), o.pop("x_right")
        return {k: v[0] for k, v in o.items()} if single else o

    def project_last_frame(self, camera, pose_curr, pose_last, pos_w, keypts, skip=None, counts=None, setup_type=SETUP_MONOCULAR, true_baseline=0.0,
                           img_bounds=None, out=None):
        """The queries of match_current_and_last_frames (projection.cc:214-262) for one pair ((15,) poses) or B pairs ((B, 15)): pos_w (m, 3) /
        (B, m, 3) = the last frame's landmark positions by key point, keypts = its undist_keypts_, skip = "!landmarks_[j] || outlier_flags_[j]".
        Returns dict(reproj, x_right, level, angle, valid, direction, num_valid); reproj / x_right / level / angle of invalid slots are not written
        (0, or the value of out[name] when the caller passes its own arrays)."""
        return self._last_frame_host(False, camera, pose_curr, pose_last, pos_w, keypts, skip, counts, setup_type, true_baseline, img_bounds, out)

    def project_last_frame_lines(self, camera, pose_curr, pose_last, pos_w, keylines, skip=None, counts=None, setup_type=SETUP_MONOCULAR,
                                 true_baseline=0.0, img_bounds=None, out=None):
        """The queries of match_current_and_last_frames_line (projection.cc:361-450): pos_w (m, 6) / (B, m, 6) start point, end point;
        keylines = the last frame's _keylsd.  Returns dict(reproj_sp, reproj_ep, x_right_sp, x_right_ep, level, valid, direction, num_valid); the end
        points of every slot are the reference's temporaries after it as DESIGN.md section 5 D6 defines them."""
        return self._last_frame_host(True, camera, pose_curr, pose_last, pos_w, keylines, skip, counts, setup_type, true_baseline, img_bounds, out)

    def _last_frame_device(self, lines, camera, B, m_cap, ptrs, setup_type, true_baseline, img_bounds, stream):
        a = _last_frame_args(camera, img_bounds, setup_type, true_baseline, B, m_cap, dev_ptrs(**ptrs))
        self._device("plp_project_last_frame_lines_device" if lines else "plp_project_last_frame_device", a, stream)

    def project_last_frame_device(self, camera, B, m_cap, pose_curr, pose_last, pos_w, keypts, out_reproj, out_level, out_valid, out_direction,
                                  skip=None, counts=None, out_x_right=None, out_angle=None, out_num_valid=None, setup_type=SETUP_MONOCULAR,
                                  true_baseline=0.0, img_bounds=None, stream=None):
        """plp_project_last_frame_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        self._last_frame_device(False, camera, B, m_cap, dict(
            pose_curr=pose_curr, pose_last=pose_last, pos_w=pos_w, keypts=keypts, skip=skip, counts=counts, out_reproj=out_reproj, out_x_right=out_x_right,
            out_level=out_level, out_angle=out_angle, out_valid=out_valid, out_direction=out_direction, out_num_valid=out_num_valid),
            setup_type, true_baseline, img_bounds, stream)

    def project_last_frame_lines_device(self, camera, B, m_cap, pose_curr, pose_last, pos_w, keylines, out_reproj_sp, out_reproj_ep, out_level,
                                        out_valid, out_direction, skip=None, counts=None, out_x_right_sp=None, out_x_right_ep=None,
                                        out_num_valid=None, setup_type=SETUP_MONOCULAR, true_baseline=0.0, img_bounds=None, stream=None):
        """plp_project_last_frame_lines_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        self._last_frame_device(True, camera, B, m_cap, dict(
            pose_curr=pose_curr, pose_last=pose_last, pos_w=pos_w, keylines=keylines, skip=skip, counts=counts, out_reproj=out_reproj_sp,
            out_reproj2=out_reproj_ep, out_x_right=out_x_right_sp, out_x_right2=out_x_right_ep, out_level=out_level, out_valid=out_valid,
            out_direction=out_direction, out_num_valid=out_num_valid), setup_type, true_baseline, img_bounds, stream)

    # ---- fuse, Sim3 and relocalisation queries: the loops in front of the searches of fuse::replace_duplication[_line], detect_duplication,
    # match_by_Sim3_transform, match_keyframes_mutually and match_frame_and_keyframe[_line] (plp_project_landmark[_line]s_*)
    def _project_host(self, lines, camera, pose, pos_w, obs_mean_normal, min_valid_dist, max_valid_dist, skip, counts, shared_landmarks, dist_mode,
                      ray_test, line_dist_mode, log_scale_factor, num_levels, img_bounds):
        pose = np.ascontiguousarray(pose, np.float64)
        single = pose.ndim == 1
        pose = pose.reshape(-1, 15)
        B = len(pose)
        w = 6 if lines else 3
        LB = 1 if shared_landmarks else B                      # problems the landmark tables hold
        pw = np.ascontiguousarray(pos_w, np.float64).reshape(LB, -1, w)
        M = pw.shape[1]
        arr = lambda v, dt, nb, *shape: None if v is None else np.ascontiguousarray(v, dt).reshape(nb, M, *shape)
        nm = None if lines else arr(obs_mean_normal, np.float64, LB, 3)
        mn, mx, sk = arr(min_valid_dist, np.float32, LB), arr(max_valid_dist, np.float32, LB), arr(skip, np.uint8, B)
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(B)
        out = dict(reproj_d=np.zeros((B, M, 2), np.float64), reproj=np.zeros((B, M, 2), np.float32), x_right=np.zeros((B, M), np.float32),
                   level=np.zeros((B, M), np.int32), valid=np.zeros((B, M), np.uint8), status=np.zeros((B, M), np.uint8), num_valid=np.zeros(B, np.int32))
        if lines:
            out.update(reproj_ep_d=np.zeros((B, M, 2), np.float64), reproj_ep=np.zeros((B, M, 2), np.float32), x_right_ep=np.zeros((B, M), np.float32))
        a = _project_args(camera, img_bounds, log_scale_factor, num_levels, B, M, shared_landmarks, dist_mode, ray_test, line_dist_mode, host_ptrs(
            empty_null=False,   # these entries check their pointers before m_cap / cap
            pose=pose, counts=cn, pos_w=pw, obs_mean_normal=nm, min_valid_dist=mn, max_valid_dist=mx, skip=sk,
            out_reproj_d=out["reproj_d"], out_reproj2_d=out.get("reproj_ep_d"), out_reproj=out["reproj"], out_reproj2=out.get("reproj_ep"),
            out_x_right=out["x_right"], out_x_right2=out.get("x_right_ep"), out_level=out["level"], out_valid=out["valid"],
            out_status=out["status"], out_num_valid=out["num_valid"]))
        self._host("plp_project_landmark_lines_host" if lines else "plp_project_landmarks_host")(a)
        if lines:
            out["reproj_sp_d"], out["reproj_sp"], out["x_right_sp"] = out.pop("reproj_d"), out.pop("reproj"), out.pop("x_right")
        return {k: v[0] for k, v in out.items()} if single else out

    def project_landmarks(self, camera, pose, pos_w, min_valid_dist, max_valid_dist, obs_mean_normal=None, skip=None, counts=None,
                          shared_landmarks=False, dist_mode=PROJECT_DIST_CENTER, ray_test=None, log_scale_factor=None, num_levels=8, img_bounds=None):
        """The queries of fuse::replace_duplication / detect_duplication, match_by_Sim3_transform, match_keyframes_mutually and
        match_frame_and_keyframe (plp_project_landmarks_host) for one problem ((15,) pose) or B ((B, 15)): pose rows from frame_pose, sim3_pose or
        mutual_poses; pos_w (m, 3) / (B, m, 3), or (m, 3) read by every problem with shared_landmarks; ray_test None = "obs_mean_normal is given".
        Returns dict(reproj_d, reproj, x_right, level, valid, status, num_valid); reproj_d / reproj / x_right / level of invalid slots are not
        written and hold 0."""
        lsf = np.float32(math.log(np.float32(1.2))) if log_scale_factor is None else log_scale_factor
        rt = (obs_mean_normal is not None) if ray_test is None else ray_test
        return self._project_host(False, camera, pose, pos_w, obs_mean_normal, min_valid_dist, max_valid_dist, skip, counts, shared_landmarks, dist_mode,
                                  rt, 0, lsf, num_levels, img_bounds)

    def project_landmark_lines(self, camera, pose, pos_w, min_valid_dist, max_valid_dist, skip=None, counts=None, shared_landmarks=False,
                               line_dist_mode=PROJECT_LINE_ENDPOINTS, log_scale_factor=None, num_levels=2, img_bounds=None):
        """The queries of fuse::replace_duplication_line (PROJECT_LINE_ENDPOINTS) and match_frame_and_keyframe_line (PROJECT_LINE_MIDPOINT)
        (plp_project_landmark_lines_host): pos_w (m, 6) / (B, m, 6) start point, end point.  Returns dict(reproj_sp_d, reproj_ep_d, reproj_sp,
        reproj_ep, x_right_sp, x_right_ep, level, valid, status, num_valid); the end points of every slot are the reference's temporaries after it as
        DESIGN.md section 5 D6 / D9 define them."""
        lsf = np.float32(math.log(np.float32(2.0))) if log_scale_factor is None else log_scale_factor
        return self._project_host(True, camera, pose, pos_w, None, min_valid_dist, max_valid_dist, skip, counts, shared_landmarks, PROJECT_DIST_CENTER,
                                  False, line_dist_mode, lsf, num_levels, img_bounds)

    def _project_device(self, lines, camera, B, m_cap, ptrs, shared_landmarks, dist_mode, ray_test, line_dist_mode, log_scale_factor, num_levels,
                        img_bounds, stream):
        a = _project_args(camera, img_bounds, log_scale_factor, num_levels, B, m_cap, shared_landmarks, dist_mode, ray_test, line_dist_mode,
                          dev_ptrs(**ptrs))
        self._device("plp_project_landmark_lines_device" if lines else "plp_project_landmarks_device", a, stream)

    def project_landmarks_device(self, camera, B, m_cap, pose, pos_w, min_valid_dist, max_valid_dist, out_valid, out_reproj_d=None, out_reproj=None,
                                 obs_mean_normal=None, skip=None, counts=None, out_x_right=None, out_level=None, out_status=None, out_num_valid=None,
                                 shared_landmarks=False, dist_mode=PROJECT_DIST_CENTER, ray_test=None, log_scale_factor=None, num_levels=8,
                                 img_bounds=None, stream=None):
        """plp_project_landmarks_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous.  The outputs
        are the q_valid / q_reproj_d / q_reproj / q_x_right / q_level of match_device."""
        lsf = np.float32(math.log(np.float32(1.2))) if log_scale_factor is None else log_scale_factor
        rt = (obs_mean_normal is not None) if ray_test is None else ray_test
        self._project_device(False, camera, B, m_cap, dict(
            pose=pose, counts=counts, pos_w=pos_w, obs_mean_normal=obs_mean_normal, min_valid_dist=min_valid_dist, max_valid_dist=max_valid_dist,
            skip=skip, out_reproj_d=out_reproj_d, out_reproj=out_reproj, out_x_right=out_x_right, out_level=out_level, out_valid=out_valid,
            out_status=out_status, out_num_valid=out_num_valid), shared_landmarks, dist_mode, rt, 0, lsf, num_levels, img_bounds, stream)

    def project_landmark_lines_device(self, camera, B, m_cap, pose, pos_w, min_valid_dist, max_valid_dist, out_valid, out_reproj_sp_d=None,
                                      out_reproj_ep_d=None, out_reproj_sp=None, out_reproj_ep=None, skip=None, counts=None, out_x_right_sp=None,
                                      out_x_right_ep=None, out_level=None, out_status=None, out_num_valid=None, shared_landmarks=False,
                                      line_dist_mode=PROJECT_LINE_ENDPOINTS, log_scale_factor=None, num_levels=2, img_bounds=None, stream=None):
        """plp_project_landmark_lines_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        lsf = np.float32(math.log(np.float32(2.0))) if log_scale_factor is None else log_scale_factor
        self._project_device(True, camera, B, m_cap, dict(
            pose=pose, counts=counts, pos_w=pos_w, min_valid_dist=min_valid_dist, max_valid_dist=max_valid_dist, skip=skip,
            out_reproj_d=out_reproj_sp_d, out_reproj2_d=out_reproj_ep_d, out_reproj=out_reproj_sp, out_reproj2=out_reproj_ep,
            out_x_right=out_x_right_sp, out_x_right2=out_x_right_ep, out_level=out_level, out_valid=out_valid, out_status=out_status,
            out_num_valid=out_num_valid), shared_landmarks, PROJECT_DIST_CENTER, False, line_dist_mode, lsf, num_levels, img_bounds, stream)

    # ---- stereo key lines: the association of the stereo constructors (frame.cc:389-427) and triangulate_stereo_for_line (frame.cc:953-1123)
    def stereo_keylines(self, keylines_left, keylines_right, train_idx, dist, counts_left=None, counts_right=None, out=None):
        """The stereo constructor's filter of the 1-NN left -> right (plp_stereo_keylines_host) for one frame ((n,) key lines, (n,) train_idx /
        dist as lbd_match_1nn returns them) or B frames ((B, cap_left) / (B, cap_right)).  Returns dict(good_match, kl_depths, kl_x_right);
        slots at or above counts_left keep 0, or the value of out[name] when the caller passes its own arrays."""
        kl = np.ascontiguousarray(keylines_left, KL_DTYPE)
        single = kl.ndim == 1
        kl = kl.reshape(1, -1) if single else kl
        B, L = kl.shape
        kr = np.ascontiguousarray(keylines_right, KL_DTYPE).reshape(B, -1)
        R = kr.shape[1]
        ti = np.ascontiguousarray(train_idx, np.int32).reshape(B, L)
        di = np.ascontiguousarray(dist, np.int32).reshape(B, L)
        cl = None if counts_left is None else np.ascontiguousarray(counts_left, np.int32).reshape(B)
        cr = None if counts_right is None else np.ascontiguousarray(counts_right, np.int32).reshape(B)
        o = out_arrays((("good_match", (B, L), np.int32), ("kl_depths", (B, L, 2), np.float32), ("kl_x_right", (B, L, 2), np.float32)), out)
        a = _struct(stereo_keylines_args_c, dict(B=B, cap_left=L, cap_right=R), dict(
            host_ptrs(keylines_left=kl, counts_left=cl, keylines_right=kr, counts_right=cr, train_idx=ti, dist=di),
            out_good_match=o["good_match"].ctypes.data, out_kl_depths=o["kl_depths"].ctypes.data, out_kl_x_right=o["kl_x_right"].ctypes.data))
        _check(lib().plp_stereo_keylines_host(self._h, C.byref(a)))
        return {k: v[0] for k, v in o.items()} if single else o

    def stereo_keylines_device(self, B, cap_left, cap_right, keylines_left, keylines_right, train_idx, dist, out_good_match, out_kl_depths,
                               out_kl_x_right, counts_left=None, counts_right=None, stream=None):
        """plp_stereo_keylines_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        a = _struct(stereo_keylines_args_c, dict(B=int(B), cap_left=int(cap_left), cap_right=int(cap_right)), dev_ptrs(
            keylines_left=keylines_left, counts_left=counts_left, keylines_right=keylines_right, counts_right=counts_right, train_idx=train_idx, dist=dist,
            out_good_match=out_good_match, out_kl_depths=out_kl_depths, out_kl_x_right=out_kl_x_right))
        self._device("plp_stereo_keylines_device", a, stream)

    def keylines_3d(self, camera, setup_type, pose, keylines, kl_depths=None, good_match=None, keylines_right=None, counts=None, counts_right=None,
                    out=None):
        """triangulate_stereo_for_line for every key line (plp_keylines_3d_host) of one frame ((15,) pose, (n,) key lines) or B frames ((B, 15),
        (B, cap)): RGB-D (SETUP_RGBD) from kl_depths (n, 2), stereo (SETUP_STEREO) from good_match (n,) and the right key lines.  camera: a
        perspective camera_model / camera_model_c.  Returns dict(pos_w (n, 6) f64, valid (n,) u8); slots at or above counts keep 0 (or out[name])."""
        pose = np.ascontiguousarray(pose, np.float64)
        single = pose.ndim == 1
        pose = pose.reshape(-1, 15)
        B = len(pose)
        kl = np.ascontiguousarray(keylines, KL_DTYPE).reshape(B, -1)
        M = kl.shape[1]
        kd = None if kl_depths is None else np.ascontiguousarray(kl_depths, np.float32).reshape(B, M, 2)
        gm = None if good_match is None else np.ascontiguousarray(good_match, np.int32).reshape(B, M)
        kr = None if keylines_right is None else np.ascontiguousarray(keylines_right, KL_DTYPE).reshape(B, -1)
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(B)
        cr = None if counts_right is None else np.ascontiguousarray(counts_right, np.int32).reshape(B)
        o = out_arrays((("pos_w", (B, M, 6), np.float64), ("valid", (B, M), np.uint8)), out)
        a = _struct(keylines_3d_args_c, dict(setup_type=int(setup_type), B=B, cap=M, cap_right=0 if kr is None else kr.shape[1]), host_ptrs(
            empty_null=False,   # these entries check their pointers before m_cap / cap
            counts=cn, pose=pose, keylines=kl, kl_depths=kd, good_match=gm, keylines_right=None if kr is None or kr.size == 0 else kr,
            counts_right=cr, out_pos_w=o["pos_w"], out_valid=o["valid"]))
        a.camera = camera_model_c.from_buffer_copy(camera)
        _check(lib().plp_keylines_3d_host(self._h, C.byref(a)))
        return {k: v[0] for k, v in o.items()} if single else o

    def keylines_3d_device(self, camera, setup_type, B, cap, pose, keylines, out_pos_w, kl_depths=None, good_match=None, keylines_right=None,
                           cap_right=0, counts=None, counts_right=None, out_valid=None, stream=None):
        """plp_keylines_3d_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        a = _struct(keylines_3d_args_c, dict(setup_type=int(setup_type), B=int(B), cap=int(cap), cap_right=int(cap_right)), dev_ptrs(
            counts=counts, pose=pose, keylines=keylines, kl_depths=kl_depths, good_match=good_match, keylines_right=keylines_right, counts_right=counts_right,
            out_pos_w=out_pos_w, out_valid=out_valid))
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_keylines_3d_device", a, stream)

    # ---- key-frame pair line triangulation: keyframe::compute_median_depth (keyframe.cc:825-857), triangulate_line_with_two_keyframes
    # (mapping_module.cc:482-601) with two_view_triangulator_line::triangulate (two_view_triangulator_line.cc:52-296)
    def median_depth(self, pose, pos_w, valid=None, counts=None, abs_flag=True):
        """compute_median_depth(abs) (plp_median_depth_host) of one key frame ((15,) pose, (m, 3) landmark positions, (m,) valid flags) or F
        key frames ((F, 15), (F, m_cap, 3), (F, m_cap)).  Returns (median f32, count i32); a key frame without a landmark gives (0.0, 0)."""
        pose = np.ascontiguousarray(pose, np.float64)
        single = pose.ndim == 1
        pose = pose.reshape(-1, 15)
        F = len(pose)
        pw = np.ascontiguousarray(pos_w, np.float64).reshape(F, -1, 3)
        M = pw.shape[1]
        va = None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(F, M)
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        med, cnt = np.zeros(F, np.float32), np.zeros(F, np.int32)
        a = _struct(median_depth_args_c, dict(F=F, m_cap=M, abs_flag=int(bool(abs_flag))), dict(
            host_ptrs(pose=pose, pos_w=pw, valid=va, counts=cn), out_median=med.ctypes.data, out_count=cnt.ctypes.data))
        _check(lib().plp_median_depth_host(self._h, C.byref(a)))
        return (med[0], cnt[0]) if single else (med, cnt)

    def median_depth_device(self, F, m_cap, pose, pos_w, out_median, out_count, valid=None, counts=None, abs_flag=True, stream=None):
        """plp_median_depth_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        a = _struct(median_depth_args_c, dict(F=int(F), m_cap=int(m_cap), abs_flag=int(bool(abs_flag))), dev_ptrs(
            pose=pose, pos_w=pos_w, valid=valid, counts=counts, out_median=out_median, out_count=out_count))
        self._device("plp_median_depth_device", a, stream)

    @staticmethod
    def _keyline_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr, dist_thr,
                              endpoint_thr, angle_thr, skip_occupied):
        keep = matcher._keypoint_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr)
        a.dist_thr, a.endpoint_thr, a.angle_thr, a.skip_occupied = float(dist_thr), float(endpoint_thr), float(angle_thr), int(bool(skip_occupied))
        return keep

    def triangulate_keyline_pairs(self, camera, setup_type, groups, keylines, line_functions, kl_x_right, pose, median_depth, occupied,
                                  scale_factors, level_sigma_sq, counts=None, kp_depths=None, kp_counts=None, lines_3d=None, lbd=None,
                                  train_idx=None, dist=None, true_baseline=0.0, scale_factor=None, rays_parallax_deg_thr=1.0, dist_thr=50.0,
                                  endpoint_thr=400.0, angle_thr=20.0, skip_occupied=True, out=None):
        """triangulate_line_with_two_keyframes over a table of F key frames (plp_triangulate_keyline_pairs_host).  groups: a list of
        (kf1, [kf2, ...]): cur against its neighbours in the reference's order.  Per key frame, leading dimension F: keylines (F, cap),
        line_functions (F, cap, 3), kl_x_right (F, cap, 2), pose (F, 15), median_depth (F,), occupied (F, cap), counts (F,), kp_depths
        (F, kp_cap) / kp_counts (F,), lines_3d (F, cap, 6) (stereo and RGB-D).  train_idx / dist (P, cap) are the 1-NN kf1 -> kf2 of every
        pair in group order; when they are not given, lbd (F, cap, 32) is matched on the device (plp_lbd_match_1nn_device, one batch).
        scale_factor: keyframe::scale_factor_ (default: scale_factors[1]).  The defaults are the mapping module's thresholds; KLP_INITIALIZER
        holds the initialiser's.  Returns dict(pairs (P, 2), group_offsets (G + 1,), train_idx, dist, match (P, cap) i32, pos_w (P, cap, 6)
        f64, status (P, cap) u8, occupied_cur (G, cap) u8); slots the kernels do not write keep 0 / -1 for match, or out[name]."""
        kl = np.ascontiguousarray(keylines, KL_DTYPE)
        if kl.ndim != 2:
            raise PlpError(PLP_ERR_INVALID_ARG, "keylines must be (F, cap)")
        F, M = kl.shape
        pairs = np.array([(int(k1), int(k2)) for k1, ngh in groups for k2 in ngh], np.int32).reshape(-1, 2)
        offs = np.zeros(len(groups) + 1, np.int32)
        offs[1:] = np.cumsum([len(ngh) for _, ngh in groups])
        Pn, G = len(pairs), len(groups)
        if Pn and (pairs.min() < 0 or pairs.max() >= F):
            raise PlpError(PLP_ERR_INVALID_ARG, "a group names a key frame outside the table")
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        if train_idx is None or dist is None:
            if lbd is None:
                raise PlpError(PLP_ERR_INVALID_ARG, "train_idx and dist, or lbd, are required")
            train_idx, dist = self._lbd_match_pairs(np.ascontiguousarray(lbd, np.uint8).reshape(F, M, 32), cn, pairs)
        ti = np.ascontiguousarray(train_idx, np.int32).reshape(Pn, M)
        di = np.ascontiguousarray(dist, np.int32).reshape(Pn, M)
        fn = np.ascontiguousarray(line_functions, np.float64).reshape(F, M, 3)
        xr = np.ascontiguousarray(kl_x_right, np.float32).reshape(F, M, 2)
        po = np.ascontiguousarray(pose, np.float64).reshape(F, 15)
        md = np.ascontiguousarray(median_depth, np.float32).reshape(F)
        oc = np.ascontiguousarray(occupied, np.uint8).reshape(F, M)
        kd = None if kp_depths is None else np.ascontiguousarray(kp_depths, np.float32).reshape(F, -1)
        kc = None if kp_counts is None else np.ascontiguousarray(kp_counts, np.int32).reshape(F)
        l3 = None if lines_3d is None else np.ascontiguousarray(lines_3d, np.float64).reshape(F, M, 6)
        o = out_arrays((("match", (Pn, M), np.int32, -1), ("pos_w", (Pn, M, 6), np.float64, 0), ("status", (Pn, M), np.uint8, 0),
                                   ("occupied_cur", (G, M), np.uint8, 0)), out)
        a = _struct(keyline_pairs_args_c, dict(F=F, cap=M, kp_cap=0 if kd is None else kd.shape[1], P=Pn, G=G), dict(
            host_ptrs(keylines=kl, counts=cn, line_functions=fn, kl_x_right=xr, kp_depths=kd, kp_counts=kc, pose=po, median_depth=md, lines_3d=l3,
                      occupied=oc, pairs=pairs, train_idx=ti, dist=di, out_match=o["match"], out_pos_w=o["pos_w"], out_status=o["status"],
                      out_occupied_cur=o["occupied_cur"]), group_offsets=offs.ctypes.data))
        keep = self._keyline_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr,
                                          dist_thr, endpoint_thr, angle_thr, skip_occupied)
        _check(lib().plp_triangulate_keyline_pairs_host(self._h, C.byref(a)))
        del keep
        return dict(pairs=pairs, group_offsets=offs, train_idx=ti, dist=di, **o)

    def _lbd_match_pairs(self, lbd, counts, pairs):
        """BinaryDescriptorMatcher::match(kf1's descriptors, kf2's) for every pair, one batched call on the device -> (train_idx, dist) (P, cap)"""
        import torch
        F, M, _ = lbd.shape
        Pn = len(pairs)
        if Pn == 0 or M == 0:
            return np.full((Pn, M), -1, np.int32), np.full((Pn, M), 256, np.int32)
        dev = torch.device("cuda", self.device)
        d = torch.from_numpy(lbd).to(dev)
        c = torch.from_numpy(np.full(F, M, np.int32) if counts is None else np.clip(counts, 0, M).astype(np.int32)).to(dev)
        pr = torch.from_numpy(pairs.astype(np.int64)).to(dev)
        q, t = d[pr[:, 0]].contiguous(), d[pr[:, 1]].contiguous()
        qc, tc = c[pr[:, 0]].contiguous(), c[pr[:, 1]].contiguous()
        idx = torch.full((Pn, M), -1, dtype=torch.int32, device=dev)
        dist = torch.full((Pn, M), 256, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().plp_lbd_match_1nn_device(self._h, q.data_ptr(), qc.data_ptr(), M, t.data_ptr(), tc.data_ptr(), M, Pn, idx.data_ptr(),
                                              dist.data_ptr(), C.c_void_p(st)))
        torch.cuda.synchronize(dev)
        return idx.cpu().numpy(), dist.cpu().numpy()

    def triangulate_keyline_pairs_device(self, camera, setup_type, F, cap, P, G, pairs, group_offsets, train_idx, dist, keylines, line_functions,
                                         kl_x_right, pose, median_depth, occupied, out_match, out_pos_w, out_status, out_occupied_cur,
                                         scale_factors, level_sigma_sq, counts=None, kp_depths=None, kp_counts=None, kp_cap=0, lines_3d=None,
                                         true_baseline=0.0, scale_factor=None, rays_parallax_deg_thr=1.0, dist_thr=50.0, endpoint_thr=400.0,
                                         angle_thr=20.0, skip_occupied=True, stream=None):
        """plp_triangulate_keyline_pairs_device: every array a device pointer (int) or a torch tensor on the matcher's device (scale_factors and
        level_sigma_sq are host vectors); asynchronous, two kernels on the stream"""
        a = _struct(keyline_pairs_args_c, dict(F=int(F), cap=int(cap), kp_cap=int(kp_cap), P=int(P), G=int(G)), dev_ptrs(
            keylines=keylines, counts=counts, line_functions=line_functions, kl_x_right=kl_x_right, kp_depths=kp_depths, kp_counts=kp_counts, pose=pose,
            median_depth=median_depth, lines_3d=lines_3d, occupied=occupied, pairs=pairs, group_offsets=group_offsets, train_idx=train_idx, dist=dist,
            out_match=out_match, out_pos_w=out_pos_w, out_status=out_status, out_occupied_cur=out_occupied_cur))
        keep = self._keyline_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr,
                                          dist_thr, endpoint_thr, angle_thr, skip_occupied)
        self._device("plp_triangulate_keyline_pairs_device", a, stream)
        del keep

    def keyframe_pair_geometry(self, camera, setup_type, pose, pairs, median_depth=None, true_baseline=0.0, out=None):
        """What create_new_landmarks computes per neighbour in front of match_for_triangulation (plp_keyframe_pair_geometry_host): pose (F, 15),
        pairs (P, 2) = (cur, ngh), median_depth (F,) f32 (monocular).  Returns dict(skip (P,) u8, epipolar (P, 12) f64, baseline (P,) f64);
        out: arrays to write into (slots the kernel does not write keep their values)."""
        po = np.ascontiguousarray(pose, np.float64).reshape(-1, 15)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        F, Pn = len(po), len(pr)
        md = None if median_depth is None else np.ascontiguousarray(median_depth, np.float32).reshape(F)
        o = out_arrays((("skip", (Pn,), np.uint8), ("epipolar", (Pn, 12), np.float64), ("baseline", (Pn,), np.float64)), out)
        a = _struct(pair_geometry_args_c, dict(F=F, P=Pn, setup_type=int(setup_type), true_baseline=float(true_baseline)), host_ptrs(
            pose=po, median_depth=md, pairs=pr, out_skip=o["skip"], out_epipolar=o["epipolar"], out_baseline=o["baseline"]))
        a.camera = camera_model_c.from_buffer_copy(camera)
        _check(lib().plp_keyframe_pair_geometry_host(self._h, C.byref(a)))
        return o

    def keyframe_pair_geometry_device(self, camera, setup_type, F, P, pose, pairs, out_skip, out_epipolar, out_baseline, median_depth=None,
                                      true_baseline=0.0, stream=None):
        """plp_keyframe_pair_geometry_device: every array a device pointer (int) or a torch tensor on the matcher's device; asynchronous"""
        a = _struct(pair_geometry_args_c, dict(F=int(F), P=int(P), setup_type=int(setup_type), true_baseline=float(true_baseline)), dev_ptrs(
            pose=pose, median_depth=median_depth, pairs=pairs, out_skip=out_skip, out_epipolar=out_epipolar, out_baseline=out_baseline))
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_keyframe_pair_geometry_device", a, stream)

    @staticmethod
    def _keypoint_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr):
        sf = np.ascontiguousarray(scale_factors, np.float32)
        ls = np.ascontiguousarray(level_sigma_sq, np.float32)
        if sf.shape != ls.shape or sf.ndim != 1:
            raise PlpError(PLP_ERR_INVALID_ARG, "scale_factors and level_sigma_sq must be vectors of the same length")
        a.camera = camera_model_c.from_buffer_copy(camera)
        a.setup_type, a.true_baseline = int(setup_type), float(true_baseline)
        a.scale_factors, a.level_sigma_sq, a.num_levels = sf.ctypes.data, ls.ctypes.data, len(sf)
        a.scale_factor = float(sf[1]) if scale_factor is None and len(sf) > 1 else float(1.0 if scale_factor is None else scale_factor)
        a.rays_parallax_deg_thr = float(rays_parallax_deg_thr)
        return sf, ls                                          # kept alive by the caller until the call has returned

    def triangulate_keypoint_pairs(self, camera, setup_type, keypts, bearings, pose, pairs, match_q, scale_factors, level_sigma_sq,
                                   x_right=None, depths=None, counts=None, q_feature=None, m_cap=None, pair_skip=None, occupied_1=None,
                                   occupied_2=None, true_baseline=0.0, scale_factor=None, rays_parallax_deg_thr=1.0, out=None):
        """two_view_triangulator::triangulate for every match of every pair (plp_triangulate_keypoint_pairs_host).  Per key frame, leading
        dimension F: keypts (F, cap) KP_DTYPE, bearings (F, cap, 3), x_right / depths (F, cap), counts (F,), pose (F, 15).  Per pair: pairs
        (P, 2) = (cur, ngh), match_q (P, cap) = the matcher's out_match, q_feature (P, m_cap) or None = identity (then m_cap defaults to cap),
        pair_skip (P,), occupied_1 / occupied_2 (P, cap) u8: updated IN PLACE when they are C-contiguous uint8 arrays.  Returns dict(idx_1
        (P, cap) i32, pos_w (P, cap, 3) f64, status (P, cap) u8, occupied_1, occupied_2); slots the kernel does not write keep -1 / 0 / 0, or
        out[name]."""
        kp = np.ascontiguousarray(keypts, KP_DTYPE)
        if kp.ndim != 2:
            raise PlpError(PLP_ERR_INVALID_ARG, "keypts must be (F, cap)")
        F, M = kp.shape
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        Pn = len(pr)
        be = np.ascontiguousarray(bearings, np.float64).reshape(F, M, 3)
        po = np.ascontiguousarray(pose, np.float64).reshape(F, 15)
        mq = np.ascontiguousarray(match_q, np.int32).reshape(Pn, M)
        qf = None if q_feature is None else np.ascontiguousarray(q_feature, np.int32).reshape(Pn, -1)
        Q = int(m_cap) if m_cap is not None else (M if qf is None else qf.shape[1])
        xr = None if x_right is None else np.ascontiguousarray(x_right, np.float32).reshape(F, M)
        de = None if depths is None else np.ascontiguousarray(depths, np.float32).reshape(F, M)
        cn = None if counts is None else np.ascontiguousarray(counts, np.int32).reshape(F)
        sk = None if pair_skip is None else np.ascontiguousarray(pair_skip, np.uint8).reshape(Pn)
        o1 = None if occupied_1 is None else np.ascontiguousarray(occupied_1, np.uint8).reshape(Pn, M)
        o2 = None if occupied_2 is None else np.ascontiguousarray(occupied_2, np.uint8).reshape(Pn, M)
        o = out_arrays((("idx_1", (Pn, M), np.int32, -1), ("pos_w", (Pn, M, 3), np.float64, 0), ("status", (Pn, M), np.uint8, 0)), out)
        a = _struct(keypoint_pairs_args_c, dict(F=F, cap=M, m_cap=Q, P=Pn), host_ptrs(
            keypts=kp, bearings=be, x_right=xr, depths=de, counts=cn, pose=po, pairs=pr, match_q=mq, q_feature=qf, pair_skip=sk, out_idx_1=o["idx_1"],
            out_pos_w=o["pos_w"], out_status=o["status"], occupied_1_io=o1, occupied_2_io=o2))
        keep = self._keypoint_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr)
        _check(lib().plp_triangulate_keypoint_pairs_host(self._h, C.byref(a)))
        del keep
        return dict(occupied_1=o1, occupied_2=o2, **o)

    def triangulate_keypoint_pairs_device(self, camera, setup_type, F, cap, m_cap, P, keypts, bearings, pose, pairs, match_q, out_idx_1,
                                          out_pos_w, out_status, scale_factors, level_sigma_sq, x_right=None, depths=None, counts=None,
                                          q_feature=None, pair_skip=None, occupied_1_io=None, occupied_2_io=None, true_baseline=0.0,
                                          scale_factor=None, rays_parallax_deg_thr=1.0, stream=None):
        """plp_triangulate_keypoint_pairs_device: every array a device pointer (int) or a torch tensor on the matcher's device (scale_factors
        and level_sigma_sq are host vectors); asynchronous, one kernel on the stream"""
        a = _struct(keypoint_pairs_args_c, dict(F=int(F), cap=int(cap), m_cap=int(m_cap), P=int(P)), dev_ptrs(
            keypts=keypts, bearings=bearings, x_right=x_right, depths=depths, counts=counts, pose=pose, pairs=pairs, match_q=match_q, q_feature=q_feature,
            pair_skip=pair_skip, out_idx_1=out_idx_1, out_pos_w=out_pos_w, out_status=out_status, occupied_1_io=occupied_1_io, occupied_2_io=occupied_2_io))
        keep = self._keypoint_pairs_params(a, camera, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr)
        self._device("plp_triangulate_keypoint_pairs_device", a, stream)
        del keep

    def landmark_geometry(self, pose, keypts, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, scale_factors, skip=None, counts=None, out=None):
        """landmark::update_normal_and_depth for L landmarks (plp_landmark_geometry_host): pose (F, 15), keypts (F, cap) KP_DTYPE, pos_w (L, 3),
        ref_kf (L,), skip (L,) u8 or None, the ragged observations obs_offsets (L + 1,) / obs_kf / obs_idx, scale_factors (num_levels,) f32.
        Returns dict(normal (L, 3) f64, min_dist / max_dist (L,) f32: the raw members, status (L,) u8: LG_*); the values are written where
        status is LG_UPDATED, elsewhere they keep 0 or out[name]."""
        return _landmark_geometry_host(self._host("plp_landmark_geometry_host"), False, pose, keypts, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx,
                                       scale_factors, None, skip, counts, out)

    def landmark_line_geometry(self, pose, keylines, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, scale_factors, scale_factors_lsd, skip=None,
                               counts=None, out=None):
        """Line::update_information for L line landmarks (plp_landmark_line_geometry_host): keylines (F, cap) KL_DTYPE, pos_w (L, 6),
        scale_factors the ORB table, scale_factors_lsd (num_levels_lsd,) the LSD table.  Returns dict(min_dist, max_dist, status)."""
        return _landmark_geometry_host(self._host("plp_landmark_line_geometry_host"), True, pose, keylines, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx,
                                       scale_factors, scale_factors_lsd, skip, counts, out)

    def _landmark_geometry_device(self, lines, F, cap, L, pose, feats, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, out_mean_normal, out_min_valid_dist,
                                  out_max_valid_dist, out_status, scale_factors, scale_factors_lsd, skip, counts, stream):
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        sl = np.ascontiguousarray(scale_factors_lsd, np.float32).reshape(-1) if lines else None    # both live until the call has returned
        a = _struct(landmark_geometry_args_c, dict(F=int(F), cap=int(cap), L=int(L), num_levels=len(sf), num_levels_lsd=len(sl) if lines else 0), dict(
            dev_ptrs(pose=pose, counts=counts, keypts=None if lines else feats, keylines=feats if lines else None, pos_w=pos_w, ref_kf=ref_kf, skip=skip,
                     obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx, out_mean_normal=out_mean_normal, out_min_valid_dist=out_min_valid_dist,
                     out_max_valid_dist=out_max_valid_dist, out_status=out_status),
            scale_factors=sf.ctypes.data, scale_factors_lsd=sl.ctypes.data if lines else None))
        self._device("plp_landmark_line_geometry_device" if lines else "plp_landmark_geometry_device", a, stream)

    def landmark_geometry_device(self, F, cap, L, pose, keypts, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, out_mean_normal, out_min_valid_dist,
                                 out_max_valid_dist, out_status, scale_factors, skip=None, counts=None, stream=None):
        """plp_landmark_geometry_device: every array a device pointer (int) or a torch tensor on the matcher's device (scale_factors is a host
        vector); asynchronous, one kernel on the stream"""
        self._landmark_geometry_device(False, F, cap, L, pose, keypts, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, out_mean_normal, out_min_valid_dist,
                                       out_max_valid_dist, out_status, scale_factors, None, skip, counts, stream)

    def landmark_line_geometry_device(self, F, cap, L, pose, keylines, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, out_min_valid_dist,
                                      out_max_valid_dist, out_status, scale_factors, scale_factors_lsd, skip=None, counts=None, stream=None):
        """plp_landmark_line_geometry_device: as landmark_geometry_device, with the LSD scale table beside the ORB one and no normal"""
        self._landmark_geometry_device(True, F, cap, L, pose, keylines, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx, None, out_min_valid_dist,
                                       out_max_valid_dist, out_status, scale_factors, scale_factors_lsd, skip, counts, stream)

    def sim3_ransac(self, camera, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, level_sigma_sq_1, level_sigma_sq_2, iters=200,
                    fix_scale=False, min_num_inliers=20, samples=None, seed=0, counts=None, outputs=None, out=None):
        """solve::sim3_solver's constructor and find_via_ransac for P problems (plp_sim3_ransac_host): valid (P, n_cap) u8, pos_w_1 / pos_w_2
        (P, n_cap, 3), octave_1 / octave_2 (P, n_cap), pose_1 / pose_2 (P, 15), the two sigma tables (num_levels,) f32, samples (P, iters, 3)
        indices of common points or None = drawn from seed, counts (P,) or None.  Returns dict(status (P,) u8: SIM3_*, num_common, rot_12
        (P, 3, 3), trans_12 (P, 3), scale_12 (P,) f32, num_inliers, best_iter, inliers (P, n_cap) u8, hyp_inliers (P, iters)); `outputs` names
        the optional ones wanted (default both); out[name]: the caller's array."""
        return _sim3_ransac_host(self._host("plp_sim3_ransac_host"), camera, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, level_sigma_sq_1,
                                 level_sigma_sq_2, iters, fix_scale, min_num_inliers, samples, seed, counts, outputs, out)

    def sim3_ransac_device(self, camera, P, n_cap, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, level_sigma_sq_1, level_sigma_sq_2, out,
                           iters=200, fix_scale=False, min_num_inliers=20, samples=None, seed=0, counts=None, stream=None):
        """plp_sim3_ransac_device: every array a device pointer (int) or a torch tensor on the matcher's device (the sigma tables are host
        vectors); out: dict of the device outputs named as in SIM3_OUTPUTS (inliers / hyp_inliers may be absent); asynchronous, three kernels
        on the stream"""
        s1 = np.ascontiguousarray(level_sigma_sq_1, np.float32).reshape(-1)
        s2 = np.ascontiguousarray(level_sigma_sq_2, np.float32).reshape(-1)        # both live until the call has returned
        a = _struct(sim3_ransac_args_c, dict(P=int(P), n_cap=int(n_cap), fix_scale=int(bool(fix_scale)), min_num_inliers=int(min_num_inliers),
                                             iters=int(iters), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, num_levels=min(len(s1), len(s2))), dict(
            dev_ptrs(counts=counts, valid=valid, pos_w_1=pos_w_1, pos_w_2=pos_w_2, octave_1=octave_1, octave_2=octave_2, pose_1=pose_1, pose_2=pose_2,
                     samples=samples), level_sigma_sq_1=host_ptr(s1), level_sigma_sq_2=host_ptr(s2)))
        set_outputs(a, SIM3_OUTPUTS, out, dev_ptr)
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_sim3_ransac_device", a, stream)

    def plane_ransac(self, mode, pos_w, flags, dist_thresh, error_thresh, points_per_ransac=18, min_points_before_ransac=12, iters=50,
                     inliers_ratio_thr=0.7, best_error_in=None, equation_in=None, samples=None, seed=0, counts=None, outputs=None, out=None):
        """Planar_Mapping_module's RANSAC for P planes (plp_plane_ransac_host): mode PLANE_CREATE (estimate_plane_sequential_RANSAC behind
        create_new_plane's gate) or PLANE_UPDATE (update_plane_via_RANSAC); pos_w (P, n_cap, 3) f64, flags (P, n_cap) u8 of PLANE_LM_*,
        dist_thresh / error_thresh a number or (P,), best_error_in (P,) / equation_in (P, 4) for UPDATE, samples (P, iters, m_cap) ranks among
        the eligible slots or None = drawn from seed, counts (P,) or None.  Returns dict(status (P,) u8: PLANE_*, flags: PLANE_FLAG_*, equation
        (P, 4), best_error, best_iter, last_iter, num_inliers, inliers (P, n_cap) u8, hyp_residual / hyp_inliers / hyp_error (P, iters));
        `outputs` names the optional ones wanted (default all); out[name]: the caller's array."""
        return _plane_ransac_host(self._host("plp_plane_ransac_host"), mode, pos_w, flags, dist_thresh, error_thresh, points_per_ransac,
                                  min_points_before_ransac, iters, inliers_ratio_thr, best_error_in, equation_in, samples, seed, counts, outputs, out)

    def plane_ransac_device(self, mode, P, n_cap, pos_w, flags, dist_thresh, error_thresh, out, points_per_ransac=18, min_points_before_ransac=12,
                            iters=50, inliers_ratio_thr=0.7, best_error_in=None, equation_in=None, samples=None, m_cap=0, seed=0, counts=None,
                            stream=None):
        """plp_plane_ransac_device: every array a device pointer (int) or a torch tensor on the matcher's device, the thresholds (P,) f64
        included; out: dict of the device outputs named as in PLANE_RANSAC_OUTPUTS (the hyp_* ones may be absent); asynchronous, two kernels
        on the stream"""
        a = _struct(plane_ransac_args_c, dict(mode=int(mode), P=int(P), n_cap=int(n_cap), points_per_ransac=int(points_per_ransac),
                                              min_points_before_ransac=int(min_points_before_ransac), iters=int(iters),
                                              inliers_ratio_thr=float(inliers_ratio_thr), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, m_cap=int(m_cap)), dev_ptrs(
            counts=counts, pos_w=pos_w, flags=flags, dist_thresh=dist_thresh, error_thresh=error_thresh, best_error_in=best_error_in, equation_in=equation_in,
            samples=samples))
        set_outputs(a, PLANE_RANSAC_OUTPUTS, out, dev_ptr)
        self._device("plp_plane_ransac_device", a, stream)

    def plane_refine_points(self, pos_w, lm_plane, flags, equation, active, dist_thresh):
        """Planar_Mapping_module::refine_points over a landmark list (plp_plane_refine_points_host): pos_w (M, 3) f64, lm_plane (M,) plane
        rows or -1, flags (M,) u8 of PLANE_LM_*, equation (NP, 4), active (NP,) u8, dist_thresh a number.  Returns (the new pos_w, changed
        (M,) u8)."""
        return _plane_refine_host(self._host("plp_plane_refine_points_host"), pos_w, lm_plane, flags, equation, active, dist_thresh)

    def plane_refine_points_device(self, M, NP, pos_w, lm_plane, flags, equation, active, dist_thresh, out_changed, stream=None):
        """plp_plane_refine_points_device: device pointers (int) or torch tensors, dist_thresh one f64 on the device; pos_w is updated in
        place; asynchronous, one kernel on the stream"""
        a = _struct(plane_refine_args_c, dict(M=int(M), NP=int(NP)), dev_ptrs(pos_w=pos_w, lm_plane=lm_plane, flags=flags, equation=equation, active=active,
                                                                              dist_thresh=dist_thresh, out_changed=out_changed))
        self._device("plp_plane_refine_points_device", a, stream)

    def plane_refinement(self, tables, dist_thresh, error_thresh, points_per_ransac=18, iters=50, dot_product_threshold=0.8, offset_delta_factor=6, seed=0,
                         stages=PLANE_STAGE_ALL, merge_cap=16, out=None):
        """Planar_Mapping_module::refinement() for G map snapshots (plp_plane_refinement_host): tables a dict of the arrays of
        PLANE_REFINEMENT_TABLES with a leading problem axis -- pl_state (G, NP_cap) u8 of PLANE_ROW_*, pl_equation (G, NP_cap, 4), pl_best_error
        (G, NP_cap) f64, pl_count (G, NP_cap), pl_lm (G, NP_cap, n_cap) i32, pos_w (G, L, 3) f64, lm_erased (G, L) u8, lm_owner (G, L) i32 --
        updated in place (an array of another type or layout is replaced in the dict); dist_thresh / error_thresh scalars or (G,); stages a mask
        of PLANE_STAGE_*.  Returns the outputs (PLANE_REFINEMENT_OUTPUTS); out: arrays to write into, whose unwritten slots keep their values."""
        return _plane_refinement_host(self._host("plp_plane_refinement_host"), tables, dist_thresh, error_thresh, points_per_ransac, iters,
                                      dot_product_threshold, offset_delta_factor, seed, stages, merge_cap, out)

    def plane_refinement_device(self, G, NP_cap, n_cap, L, tables, dist_thresh, error_thresh, out, points_per_ransac=18, iters=50, dot_product_threshold=0.8,
                                offset_delta_factor=6, seed=0, stages=PLANE_STAGE_ALL, merge_cap=16, stream=None):
        """plp_plane_refinement_device: every array a device pointer (int) or a torch tensor on the matcher's device, the thresholds (G,) f64
        tensors, `tables` and `out` dicts named as PLANE_REFINEMENT_TABLES / PLANE_REFINEMENT_OUTPUTS (all required; merges may be absent when
        merge_cap is 0); asynchronous on `stream`"""
        a = _struct(plane_refinement_args_c, dict(G=int(G), NP_cap=int(NP_cap), n_cap=int(n_cap), L=int(L), merge_cap=int(merge_cap), stages=int(stages),
                                                  points_per_ransac=int(points_per_ransac), iters=int(iters), offset_delta_factor=int(offset_delta_factor),
                                                  dot_product_threshold=float(dot_product_threshold), seed=int(seed) & 0xFFFFFFFFFFFFFFFF),
                    dev_ptrs(dist_thresh=dist_thresh, error_thresh=error_thresh, **{k: tables[k] for k in PLANE_REFINEMENT_TABLES}))
        set_outputs(a, PLANE_REFINEMENT_OUTPUTS, out, dev_ptr)
        self._device("plp_plane_refinement_device", a, stream)

    def pnp_ransac(self, valid, bearing, pos_w, octave, scale_factors, iters=30, min_num_inliers=10, recompute=True, samples=None, seed=0, counts=None,
                   outputs=None, out=None):
        """solve::pnp_solver's constructor and find_via_ransac for P problems (plp_pnp_ransac_host): valid (P, n_cap) u8, bearing / pos_w
        (P, n_cap, 3) f64, octave (P, n_cap), scale_factors (num_levels,) f32, samples (P, iters, 4) indices of matches or None = drawn from
        seed, counts (P,) or None.  Returns dict(status (P,) u8: PNP_*, num_matches, rot_cw (P, 3, 3), trans_cw (P, 3), num_inliers, best_iter,
        inliers (P, n_cap) u8, hyp_inliers (P, iters)); `outputs` names the optional ones wanted (default both); out[name]: the caller's array."""
        return _pnp_ransac_host(self._host("plp_pnp_ransac_host"), valid, bearing, pos_w, octave, scale_factors, iters, min_num_inliers, recompute, samples,
                                seed, counts, outputs, out)

    def pnp_ransac_device(self, P, n_cap, valid, bearing, pos_w, octave, scale_factors, out, iters=30, min_num_inliers=10, recompute=True, samples=None,
                          seed=0, counts=None, stream=None):
        """plp_pnp_ransac_device: every array a device pointer (int) or a torch tensor on the matcher's device (scale_factors is a host vector);
        out: dict of the device outputs named as in PNP_OUTPUTS (inliers / hyp_inliers may be absent); asynchronous, five kernels on the stream"""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)           # lives until the call has returned
        a = _struct(pnp_ransac_args_c, dict(P=int(P), n_cap=int(n_cap), min_num_inliers=int(min_num_inliers), iters=int(iters),
                                            recompute=int(bool(recompute)), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, num_levels=len(sf)), dict(
            dev_ptrs(counts=counts, valid=valid, bearing=bearing, pos_w=pos_w, octave=octave, samples=samples), scale_factors=host_ptr(sf)))
        set_outputs(a, PNP_OUTPUTS, out, dev_ptr)
        self._device("plp_pnp_ransac_device", a, stream)

    def essential_ransac(self, bearing_1, bearing_2, match, iters=100, recompute=True, samples=None, seed=0, counts_1=None, counts_2=None, outputs=None,
                         out=None):
        """solve::essential_solver's find_via_ransac for P pairs of frames (plp_essential_ransac_host): bearing_1
        (P, n_cap, 3) / bearing_2 (P, m_cap, 3) f64, match (P, n_cap) i32: the index in frame 2 or a negative number, samples (P, iters, 8)
        indices of matches or None = drawn from seed, counts_1 / counts_2 (P,) or None.  Returns dict(status (P,) u8: ESSENTIAL_*, num_matches,
        E_21 (P, 3, 3), score (P,) f32, num_inliers, best_iter, inliers (P, n_cap) u8, hyp_score (P, iters) f32); `outputs` names the optional
        ones wanted (default both); out[name]: the caller's array."""
        return _essential_ransac_host(self._host("plp_essential_ransac_host"), bearing_1, bearing_2, match, iters, recompute, samples, seed, counts_1, counts_2,
                                      outputs, out)

    def essential_ransac_device(self, P, n_cap, m_cap, bearing_1, bearing_2, match, out, iters=100, recompute=True, samples=None, seed=0, counts_1=None,
                                counts_2=None, stream=None):
        """plp_essential_ransac_device: every array a device pointer (int) or a torch tensor on the matcher's device; out: dict of the device
        outputs named as in ESSENTIAL_OUTPUTS (inliers / hyp_score may be absent); asynchronous, five kernels on the stream"""
        a = _struct(essential_ransac_args_c, dict(P=int(P), n_cap=int(n_cap), m_cap=int(m_cap), iters=int(iters), recompute=int(bool(recompute)),
                                                  seed=int(seed) & 0xFFFFFFFFFFFFFFFF),
                    dev_ptrs(counts_1=counts_1, counts_2=counts_2, bearing_1=bearing_1, bearing_2=bearing_2, match=match, samples=samples))
        set_outputs(a, ESSENTIAL_OUTPUTS, out, dev_ptr)
        self._device("plp_essential_ransac_device", a, stream)

    def perspective_ransac(self, undist_1, undist_2, match, iters=100, recompute=True, samples_h=None, samples_f=None, seed=0, counts_1=None, counts_2=None,
                           given_H_21=None, given_H_num_inliers=None, outputs=None, out=None):
        """The homography and the fundamental RANSAC of initialize::perspective::initialize and the choice between them for P pairs of frames
        (plp_perspective_ransac_host): undist_1 (P, n_cap) / undist_2 (P, m_cap) key points (KP_DTYPE records, or (.., 2)
        points), match (P, n_cap) i32: the index in frame 2 or a negative number, samples_h / samples_f (P, iters, 8) indices of matches or None =
        drawn from seed, counts_1 / counts_2 (P,) or None, given_H_21 (P, 3, 3) with given_H_num_inliers (P,): the homography of the caller's own
        RANSAC for the problems whose count is not negative.  Returns a dict named as PERSPECTIVE_RANSAC_OUTPUTS; `outputs` names the optional ones
        wanted (default all); out[name]: the caller's array."""
        return _perspective_ransac_host(self._host("plp_perspective_ransac_host"), undist_1, undist_2, match, iters, recompute, samples_h, samples_f, seed,
                                        counts_1, counts_2, given_H_21, given_H_num_inliers, outputs, out)

    def perspective_ransac_device(self, P, n_cap, m_cap, undist_1, undist_2, match, out, iters=100, recompute=True, samples_h=None, samples_f=None, seed=0,
                                  counts_1=None, counts_2=None, given_H_21=None, given_H_num_inliers=None, stream=None):
        """plp_perspective_ransac_device: every array a device pointer (int) or a torch tensor on the matcher's device (the key points as bytes of
        KP_DTYPE records); out: dict of the device outputs named as in PERSPECTIVE_RANSAC_OUTPUTS (the optional ones may be absent); asynchronous,
        five kernels on the stream"""
        a = _struct(perspective_ransac_args_c, dict(P=int(P), n_cap=int(n_cap), m_cap=int(m_cap), iters=int(iters), recompute=int(bool(recompute)),
                                                    seed=int(seed) & 0xFFFFFFFFFFFFFFFF),
                    dev_ptrs(counts_1=counts_1, counts_2=counts_2, undist_1=undist_1, undist_2=undist_2, match=match, samples_h=samples_h, samples_f=samples_f,
                             given_H_21=given_H_21, given_H_num_inliers=given_H_num_inliers))
        set_outputs(a, PERSPECTIVE_RANSAC_OUTPUTS, out, dev_ptr)
        self._device("plp_perspective_ransac_device", a, stream)

    def perspective_pose(self, camera, choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated=50,
                         parallax_deg_thr=1.0, reproj_err_thr=4.0, counts_1=None, counts_2=None, img_bounds=None, outputs=None, out=None):
        """perspective::reconstruct_with_H / reconstruct_with_F for P frame pairs (plp_perspective_pose_host): camera a
        camera_model of the perspective or fisheye model, choice (P,) u8, H_21 / F_21 (P, 3, 3), inliers (P, n_cap) u8 and match (P, n_cap) i32 as
        matcher.perspective_ransac gives and takes them, bearing_1 (P, n_cap, 3) / bearing_2 (P, m_cap, 3), undist_1 / undist_2 the key points.
        Returns a dict named as PERSPECTIVE_POSE_OUTPUTS (status: TWO_VIEW_* or PERSPECTIVE_POSE_NO_DECOMPOSITION; num_valid / parallax_deg (P, 8));
        `outputs` names the optional ones wanted; out[name]: the caller's array."""
        return _perspective_pose_host(self._host("plp_perspective_pose_host"), camera, choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2,
                                      min_num_triangulated, parallax_deg_thr, reproj_err_thr, counts_1, counts_2, img_bounds, outputs, out)

    def perspective_pose_device(self, camera, P, n_cap, m_cap, choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, out,
                                min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, counts_1=None, counts_2=None, img_bounds=None, stream=None):
        """plp_perspective_pose_device: every array a device pointer (int) or a torch tensor on the matcher's device; out: dict of the device outputs
        named as in PERSPECTIVE_POSE_OUTPUTS (hyp_is_triangulated may be absent); asynchronous, one kernel on the stream"""
        a = perspective_pose_args(camera, dict(P=int(P), n_cap=int(n_cap), m_cap=int(m_cap), min_num_triangulated=int(min_num_triangulated),
                                               parallax_deg_thr=float(parallax_deg_thr), reproj_err_thr=float(reproj_err_thr)),
                                  dev_ptrs(counts_1=counts_1, counts_2=counts_2, in_choice=choice, H_21=H_21, F_21=F_21, inliers=inliers, match=match,
                                           bearing_1=bearing_1, bearing_2=bearing_2, undist_1=undist_1, undist_2=undist_2), img_bounds)
        set_outputs(a, PERSPECTIVE_POSE_OUTPUTS, out, dev_ptr)
        self._device("plp_perspective_pose_device", a, stream)

    def two_view_pose(self, camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, min_num_triangulated=50, parallax_deg_thr=1.0,
                      reproj_err_thr=4.0, depth_is_positive=False, in_status=None, counts_1=None, counts_2=None, img_bounds=None, outputs=None, out=None):
        """bearing_vector::reconstruct_with_E for P frame pairs (plp_two_view_pose_host): camera a camera_model, E_21
        (P, 3, 3), inliers (P, n_cap) u8 and match (P, n_cap) i32 as matcher.essential_ransac gives and takes them, bearing_1 (P, n_cap, 3) /
        bearing_2 (P, m_cap, 3), undist_1 (P, n_cap) / undist_2 (P, m_cap) KP_DTYPE, in_status (P,) u8 or None: the RANSAC's status.  Returns
        dict(status (P,) u8: TWO_VIEW_*, rot_ref_to_cur (P, 3, 3), trans_ref_to_cur (P, 3), hypothesis, num_valid (P, 4), parallax_deg (P, 4) f32,
        triangulated_pts (P, n_cap, 3), is_triangulated (P, n_cap) u8, hyp_is_triangulated (P, 4, n_cap) u8)."""
        return _two_view_pose_host(self._host("plp_two_view_pose_host"), camera, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2,
                                   min_num_triangulated, parallax_deg_thr, reproj_err_thr, depth_is_positive, in_status, counts_1, counts_2, img_bounds, outputs, out)

    def two_view_pose_device(self, camera, P, n_cap, m_cap, E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2, out, min_num_triangulated=50,
                             parallax_deg_thr=1.0, reproj_err_thr=4.0, depth_is_positive=False, in_status=None, counts_1=None, counts_2=None, img_bounds=None,
                             stream=None):
        """plp_two_view_pose_device: every array a device pointer (int) or a torch tensor on the matcher's device; out: dict of the device outputs
        named as in TWO_VIEW_OUTPUTS (hyp_is_triangulated may be absent); asynchronous, one kernel on the stream"""
        a = two_view_args(camera, dict(P=int(P), n_cap=int(n_cap), m_cap=int(m_cap), min_num_triangulated=int(min_num_triangulated),
                                       parallax_deg_thr=float(parallax_deg_thr), reproj_err_thr=float(reproj_err_thr), depth_is_positive=int(bool(depth_is_positive))),
                          dev_ptrs(counts_1=counts_1, counts_2=counts_2, in_status=in_status, E_21=E_21, inliers=inliers, match=match, bearing_1=bearing_1,
                                   bearing_2=bearing_2, undist_1=undist_1, undist_2=undist_2), img_bounds)
        set_outputs(a, TWO_VIEW_OUTPUTS, out, dev_ptr)
        self._device("plp_two_view_pose_device", a, stream)

    def pose_optimize(self, camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right=None, counts=None, lines=None, num_trials=4,
                      num_each_iter=10, outputs=None, out=None):
        """optimize::pose_optimizer::optimize (lines None) / pose_optimizer_extended_line::optimize for B frames (plp_pose_optimize_host): camera a
        camera_model, setup_type 0 / 1 / 2, pose_in (B, >= 12) rot_cw row-major + trans_cw (frame_pose rows), valid (B, n_cap) u8, undist (B, n_cap)
        KP_DTYPE, pos_w (B, n_cap, 3), inv_level_sigma_sq (num_levels,) f32, x_right (B, n_cap) f32 or None = monocular key points, counts (B,) or
        None; lines: dict(valid (B, l_cap), keylines KL_DTYPE, pos_w (B, l_cap, 6) Pluecker, inv_level_sigma_sq_lsd, counts or None).  Returns
        dict(status (B,) u8: POSE_OPT_*, pose (B, 15), num_init_obs, num_valid, outlier (B, n_cap) u8, outlier_lines (B, l_cap), trial_info
        (B, num_trials, 4), trial_chi2 (B, num_trials, 2)); `outputs` names the optional ones wanted (default both); out[name]: the caller's array
        (slots the reference does not write keep their values)."""
        return _pose_optimize_host(self._host("plp_pose_optimize_host"), camera, setup_type, pose_in, valid, undist, pos_w, inv_level_sigma_sq, x_right, counts,
                                   lines, num_trials, num_each_iter, outputs, out)

    def pose_optimize_device(self, camera, setup_type, B, n_cap, pose_in, valid, undist, pos_w, inv_level_sigma_sq, out, x_right=None, counts=None,
                             l_cap=0, line_valid=None, keylines=None, pos_w_lines=None, inv_level_sigma_sq_lsd=None, line_counts=None, num_trials=4,
                             num_each_iter=10, pose_stride=15, stream=None):
        """plp_pose_optimize_device: every array a device pointer (int) or a torch tensor on the matcher's device (the two sigma tables are host
        vectors); out: dict of the device outputs named as in POSE_OPT_OUTPUTS (trial_info / trial_chi2 may be absent, outlier_lines when l_cap
        is 0); asynchronous, two kernels on the stream"""
        sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)           # live until the call has returned
        sl = None if inv_level_sigma_sq_lsd is None else np.ascontiguousarray(inv_level_sigma_sq_lsd, np.float32).reshape(-1)
        a = _struct(pose_optimize_args_c, dict(setup_type=int(setup_type), B=int(B), n_cap=int(n_cap), l_cap=int(l_cap), num_trials=int(num_trials),
                                               num_each_iter=int(num_each_iter), pose_stride=int(pose_stride), num_levels=len(sg),
                                               num_levels_lsd=0 if sl is None else len(sl)), dict(
            dev_ptrs(pose_in=pose_in, counts=counts, line_counts=line_counts, valid=valid, undist=undist, x_right=x_right, pos_w=pos_w, line_valid=line_valid,
                     keylines=keylines, pos_w_lines=pos_w_lines), inv_level_sigma_sq=host_ptr(sg),
            inv_level_sigma_sq_lsd=host_ptr(sl)))
        set_outputs(a, POSE_OPT_OUTPUTS, out, dev_ptr)
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_pose_optimize_device", a, stream)

    def transform_optimize(self, camera, fix_scale, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2, rot_12, trans_12, scale_12,
                           inv_level_sigma_sq_1, inv_level_sigma_sq_2, counts=None, num_iter=10, chi_sq=10.0, outputs=None, out=None):
        """optimize::transform_optimizer::optimize for P pairs (plp_transform_optimize_host): camera a camera_model, valid (P, n_cap) u8, pos_w_1 / pos_w_2
        (P, n_cap, 3), undist_1 / undist_2 (P, n_cap) KP_DTYPE, pose_1 / pose_2 (P, 15) pose rows, rot_12 (P, 9), trans_12 (P, 3), scale_12 (P,) f32, the two
        sigma tables (num_levels,) f32, counts (P,) or None.  Returns dict(status (P,) u8: TRANSFORM_OPT_*, num_valid, num_inliers, rot_12, trans_12,
        scale_12 (P,) f64, world_to_1 (P, 13), kept (P, n_cap) u8, round_info (P, 2, 4), round_chi2 (P, 2, 2)); `outputs` names the optional ones wanted
        (default all); out[name]: the caller's array (slots the reference does not write keep their values)."""
        call = self._host("plp_transform_optimize_host")
        inputs = dict(camera=camera, fix_scale=fix_scale, valid=valid, pos_w_1=pos_w_1, pos_w_2=pos_w_2, undist_1=undist_1, undist_2=undist_2, pose_1=pose_1,
                      pose_2=pose_2, rot_12=rot_12, trans_12=trans_12, scale_12=scale_12, inv_level_sigma_sq_1=inv_level_sigma_sq_1,
                      inv_level_sigma_sq_2=inv_level_sigma_sq_2, counts=counts, num_iter=num_iter, chi_sq=chi_sq)
        return _transform_optimize_host(call, inputs, outputs, out)

    def transform_optimize_device(self, camera, fix_scale, P, n_cap, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2, rot_12, trans_12, scale_12,
                                  inv_level_sigma_sq_1, inv_level_sigma_sq_2, out, counts=None, num_iter=10, chi_sq=10.0, stream=None):
        """plp_transform_optimize_device: every array a device pointer (int) or a torch tensor on the matcher's device (the two sigma tables are host
        vectors); out: dict of the device outputs named as in TRANSFORM_OPT_OUTPUTS (world_to_1 / round_info / round_chi2 may be absent); asynchronous,
        three kernels on the stream"""
        s1 = np.ascontiguousarray(inv_level_sigma_sq_1, np.float32).reshape(-1)         # live until the call has returned
        s2 = np.ascontiguousarray(inv_level_sigma_sq_2, np.float32).reshape(-1)
        if len(s1) != len(s2):
            raise PlpError(PLP_ERR_INVALID_ARG, "the two sigma tables must have one length")
        a = _struct(transform_optimize_args_c, dict(fix_scale=int(bool(fix_scale)), num_iter=int(num_iter), chi_sq=float(chi_sq), P=int(P), n_cap=int(n_cap),
                                                    num_levels=len(s1)), dict(
            dev_ptrs(counts=counts, valid=valid, pos_w_1=pos_w_1, pos_w_2=pos_w_2, undist_1=undist_1, undist_2=undist_2, pose_1=pose_1, pose_2=pose_2,
                     rot_12=rot_12, trans_12=trans_12, scale_12=scale_12), inv_level_sigma_sq_1=host_ptr(s1), inv_level_sigma_sq_2=host_ptr(s2)))
        set_outputs(a, TRANSFORM_OPT_OUTPUTS, out, dev_ptr)
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_transform_optimize_device", a, stream)

    def local_ba(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right=None, counts=None,
                 kf_erased=None, kf_is_origin=None, lm_erased=None, num_first_iter=5, num_second_iter=10, outputs=None, out=None):
        """optimize::local_bundle_adjuster::optimize for G problems over shared map tables (plp_local_ba_host): camera a
        camera_model, pose (F, >= 12), undist (F, kp_stride) KP_DTYPE, x_right (F, kp_stride) f32 or None, counts (F,) or None, pos_w (L, 3), the
        observation lists obs_offsets (L + 1,), obs_kf / obs_idx (T,), kf_local (G, F) u8, the sigma table (num_levels,) f32, kf_erased / kf_is_origin (F,)
        and lm_erased (L,) u8 or None.  Returns dict(status (G,) u8: LOCAL_BA_*, kf_role (G, F), lm_role (G, L), pose (G, F, 15), pos_w (G, L, 3),
        outlier (G, T), round_info (G, 2, 4), round_chi2 (G, 2, 2)); `outputs` names the optional ones wanted (default all); out[name]: the caller's
        array (slots the adjuster does not write keep their values)."""
        return _local_ba_host(self._host("plp_local_ba_host"), _local_ba_kw(
            camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin,
            lm_erased, num_first_iter, num_second_iter), outputs, out)

    def local_ba_device(self, camera, setup_type, G, F, L, T, kp_stride, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, out,
                        x_right=None, counts=None, kf_erased=None, kf_is_origin=None, lm_erased=None, pose_stride=15, num_first_iter=5, num_second_iter=10,
                        stream=None):
        """plp_local_ba_device: every array a device pointer (int) or a torch tensor on the matcher's device (the sigma table is a host vector); out: dict
        of the device outputs named as in LOCAL_BA_OUTPUTS (round_info / round_chi2 may be absent); asynchronous, three kernels on the stream"""
        sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)             # live until the call has returned
        a = _struct(local_ba_args_c, dict(setup_type=int(setup_type), num_first_iter=int(num_first_iter), num_second_iter=int(num_second_iter), G=int(G), F=int(F),
                                          L=int(L), T=int(T), kp_stride=int(kp_stride), pose_stride=int(pose_stride), num_levels=len(sg)), dict(
            dev_ptrs(pose=pose, kf_erased=kf_erased, kf_is_origin=kf_is_origin, undist=undist, x_right=x_right, counts=counts, pos_w=pos_w,
                     lm_erased=lm_erased, obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx, kf_local=kf_local), inv_level_sigma_sq=host_ptr(sg)))
        set_outputs(a, LOCAL_BA_OUTPUTS, out, dev_ptr)
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_local_ba_device", a, stream)

    def local_ba_lines(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, keylines, pluecker,
                       obs_offsets_lines, obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, x_right=None, counts=None, kf_erased=None, kf_is_origin=None,
                       lm_erased=None, kl_counts=None, line_erased=None, num_first_iter=5, num_second_iter=10, outputs=None, out=None):
        """optimize::local_bundle_adjuster_extended_line::optimize for G problems over shared map tables (plp_local_ba_lines_host):
        local_ba's arguments, and keylines (F, kl_stride) KL_DTYPE, pluecker (LL, 6), the lines' observation lists obs_offsets_lines (LL + 1,), obs_kf_lines /
        obs_idx_lines (TL,), the lsd sigma table, kl_counts (F,) and line_erased (LL,) or None.  Returns local_ba's dict and line_role (G, LL), pluecker
        (G, LL, 6), outlier_lines (G, TL)."""
        return _local_ba_lines_host(self._host("plp_local_ba_lines_host"), _local_ba_lines_kw(
            camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq, keylines, pluecker, obs_offsets_lines, obs_kf_lines,
            obs_idx_lines, inv_level_sigma_sq_lsd, x_right, counts, kf_erased, kf_is_origin, lm_erased, kl_counts, line_erased, num_first_iter, num_second_iter),
            outputs, out)

    def local_ba_lines_device(self, camera, setup_type, G, F, L, T, kp_stride, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, kf_local, inv_level_sigma_sq,
                              LL, TL, kl_stride, keylines, pluecker, obs_offsets_lines, obs_kf_lines, obs_idx_lines, inv_level_sigma_sq_lsd, out, x_right=None,
                              counts=None, kf_erased=None, kf_is_origin=None, lm_erased=None, kl_counts=None, line_erased=None, pose_stride=15, num_first_iter=5,
                              num_second_iter=10, stream=None):
        """plp_local_ba_lines_device: every array a device pointer (int) or a torch tensor on the matcher's device (the two sigma tables are host vectors);
        out: dict of the device outputs named as in LOCAL_BA_OUTPUTS and LOCAL_BA_LINES_OUTPUTS (round_info / round_chi2 may be absent); asynchronous,
        four kernels on the stream"""
        sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)             # live until the call has returned
        sl = np.ascontiguousarray(inv_level_sigma_sq_lsd, np.float32).reshape(-1)
        pa = _struct(local_ba_args_c, dict(setup_type=int(setup_type), num_first_iter=int(num_first_iter), num_second_iter=int(num_second_iter), G=int(G), F=int(F),
                                           L=int(L), T=int(T), kp_stride=int(kp_stride), pose_stride=int(pose_stride), num_levels=len(sg)), dict(
            dev_ptrs(pose=pose, kf_erased=kf_erased, kf_is_origin=kf_is_origin, undist=undist, x_right=x_right, counts=counts, pos_w=pos_w,
                     lm_erased=lm_erased, obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx, kf_local=kf_local), inv_level_sigma_sq=host_ptr(sg)))
        set_outputs(pa, LOCAL_BA_OUTPUTS, out, dev_ptr)
        pa.camera = camera_model_c.from_buffer_copy(camera)
        a = _struct(local_ba_lines_args_c, dict(LL=int(LL), TL=int(TL), kl_stride=int(kl_stride), num_levels_lsd=len(sl)), dict(
            dev_ptrs(keylines=keylines, kl_counts=kl_counts, pluecker=pluecker, line_erased=line_erased, obs_offsets_lines=obs_offsets_lines,
                     obs_kf_lines=obs_kf_lines, obs_idx_lines=obs_idx_lines), inv_level_sigma_sq_lsd=host_ptr(sl)))
        a.points = pa
        set_outputs(a, LOCAL_BA_LINES_OUTPUTS, out, dev_ptr)
        self._device("plp_local_ba_lines_device", a, stream)

    def pose_graph_optimize(self, tables, problems, edge_cap=POSE_GRAPH_MAX_EDGES, env_cap=POSE_GRAPH_MAX_ENV, max_iter=50, outputs=None, out=None):
        """optimize::graph_optimizer::optimize for G problems over one key-frame table (plp_pose_graph_optimize_host): tables a dict of
        POSE_GRAPH_TABLES (pose (F, >= 12), kf_parent, D21's kf_conn / kf_conn_w / kf_n_conn / kf_covis / kf_covis_w / kf_n_covis, the loop edges kf_loop_offsets
        (F + 1,) / kf_loop; kf_erased, kf_id (default: the row) optional), problems a list of dicts (pose_graph_problems) or its arrays.  Returns dict(status (G,)
        u8: POSE_GRAPH_*, num_edges (G,), edges (G, edge_cap, 3), sim3_cw, corrected_wc (G, F, 8), pose (G, F, 15), info (G, 4), chi2 (G, 2)); `outputs` names
        the optional ones wanted (default all); out[name]: the caller's array (slots the optimizer does not write keep their values)."""
        return _pose_graph_host(self._host("plp_pose_graph_optimize_host"), tables, problems, edge_cap, env_cap, max_iter, outputs, out)

    def pose_graph_optimize_device(self, G, F, tables, problems, out, conn_cap, covis_cap, edge_cap, env_cap, pose_stride=15, max_iter=50, stream=None):
        """plp_pose_graph_optimize_device: tables / problems: dicts of device pointers (int) or torch tensors on the matcher's device named as POSE_GRAPH_TABLES and
        as pose_graph_problems() names them; out: dict of the device outputs named as in POSE_GRAPH_OUTPUTS (all but status may be absent); asynchronous, three
        kernels on the stream"""
        a = _struct(pose_graph_args_c, dict(G=int(G), F=int(F), pose_stride=int(pose_stride), conn_cap=int(conn_cap), covis_cap=int(covis_cap), edge_cap=int(edge_cap),
                                            env_cap=int(env_cap), max_iter=int(max_iter)), {**{k: dev_ptr(tables.get(k)) for k in POSE_GRAPH_TABLES},
                                                                                            **{k: dev_ptr(v) for k, v in problems.items()}})
        set_outputs(a, POSE_GRAPH_OUTPUTS, out, dev_ptr)
        self._device("plp_pose_graph_optimize_device", a, stream)

    def correct_landmarks(self, pos_w, ref_kf, sim3_cw, corrected_wc, lm_erased=None, kf_erased=None, out=None):
        """The landmark half of graph_optimizer::optimize (:331-350; plp_correct_landmarks_host): pos_w (L, 3), ref_kf (L,) the row each landmark is corrected
        with, sim3_cw / corrected_wc (F, 8) one problem's outputs of pose_graph_optimize.  Returns dict(pos_w (L, 3), status (L,) u8: CORRECT_LM_*); out[name]:
        the caller's array (a landmark that is not corrected keeps its slot)."""
        return _correct_landmarks_host(self._host("plp_correct_landmarks_host"), pos_w, ref_kf, sim3_cw, corrected_wc, lm_erased, kf_erased, out)

    def correct_landmarks_device(self, L, F, pos_w, ref_kf, sim3_cw, corrected_wc, out_pos_w, out_status, lm_erased=None, kf_erased=None, stream=None):
        """plp_correct_landmarks_device: device pointers (int) or torch tensors; out_pos_w may be pos_w; asynchronous"""
        a = _struct(correct_landmarks_args_c, dict(L=int(L), F=int(F)), dev_ptrs(pos_w=pos_w, lm_erased=lm_erased, ref_kf=ref_kf, kf_erased=kf_erased,
                                                                                 sim3_cw=sim3_cw, corrected_wc=corrected_wc, out_pos_w=out_pos_w,
                                                                                 out_status=out_status))
        self._device("plp_correct_landmarks_device", a, stream)

    def global_ba(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right=None, counts=None, kf_erased=None,
                  kf_is_origin=None, lm_erased=None, num_iter=10, use_huber_kernel=True, stop=None, outputs=None, out=None):
        """optimize::global_bundle_adjuster::optimize over the whole point map (plp_global_ba_host): the tables of local_ba without
        kf_local; stop: None or an int32 array of one element (force_stop_flag).  Returns dict(status (1,) u8: GLOBAL_BA_*, kf_optimized (F,), lm_optimized (L,),
        pose (F, 15), pos_w (L, 3), info (4,), chi2 (3,)); `outputs` names the optional ones wanted (default all); out[name]: the caller's array (slots the
        adjuster does not write keep their values)."""
        return _global_ba_host(self._host("plp_global_ba_host"), _global_ba_kw(
            camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin, lm_erased, num_iter,
            use_huber_kernel, stop), outputs, out)

    def global_ba_device(self, camera, setup_type, F, L, T, kp_stride, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, out, x_right=None,
                         counts=None, kf_erased=None, kf_is_origin=None, lm_erased=None, pose_stride=15, num_iter=10, use_huber_kernel=True, stop=None, stream=None):
        """plp_global_ba_device: every array a device pointer (int) or a torch tensor on the matcher's device (the sigma table is a host vector, stop None or a
        host int32 array of one element); out: dict of the device outputs named as in GLOBAL_BA_OUTPUTS (info / chi2 may be absent).  SYNCHRONOUS with respect to
        the stream: the entry reads the run's record back after every try; it returns when the outputs are written."""
        sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)             # live until the call has returned
        a = _struct(global_ba_args_c, dict(setup_type=int(setup_type), num_iter=int(num_iter), use_huber_kernel=int(bool(use_huber_kernel)), F=int(F), L=int(L), T=int(T),
                                           kp_stride=int(kp_stride), pose_stride=int(pose_stride), num_levels=len(sg)), dict(
            dev_ptrs(pose=pose, kf_erased=kf_erased, kf_is_origin=kf_is_origin, undist=undist, x_right=x_right, counts=counts, pos_w=pos_w, lm_erased=lm_erased,
                     obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx), inv_level_sigma_sq=host_ptr(sg), stop=host_ptr(stop)))
        set_outputs(a, GLOBAL_BA_OUTPUTS, out, dev_ptr)
        a.camera = camera_model_c.from_buffer_copy(camera)
        self._device("plp_global_ba_device", a, stream)

    def loop_ba_propagate(self, pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized, pos_after, kf_erased=None, kf_is_origin=None,
                          lm_erased=None, out=None):
        """The loop adjuster's map update (module/loop_bundle_adjuster.cc:109-181; plp_loop_ba_propagate_host): pose (F, >= 12) before the correction, kf_parent
        (F,), the adjuster's kf_optimized / pose (F, 15) / lm_optimized / pos_w, the landmarks' pos_w and ref_kf.  Returns dict(pose (F, 15), pose_before (F, 12),
        kf_status (F,) u8: LOOP_BA_KF_*, pos_w (L, 3), lm_status (L,) u8: LOOP_BA_LM_*); out[name]: the caller's array (rows that are not written keep their values)."""
        return _loop_ba_propagate_host(self._host("plp_loop_ba_propagate_host"), pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized, pos_after,
                                       kf_erased, kf_is_origin, lm_erased, out)

    def loop_ba_propagate_device(self, F, L, pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized, pos_after, out, kf_erased=None, kf_is_origin=None,
                                 lm_erased=None, pose_stride=15, stream=None):
        """plp_loop_ba_propagate_device: device pointers (int) or torch tensors; out: dict of the device outputs named as in LOOP_BA_PROPAGATE_OUTPUTS; asynchronous"""
        a = _struct(loop_ba_propagate_args_c, dict(F=int(F), L=int(L), pose_stride=int(pose_stride)), dev_ptrs(
            pose=pose, kf_erased=kf_erased, kf_is_origin=kf_is_origin, kf_parent=kf_parent, kf_optimized=kf_optimized, pose_after=pose_after, pos_w=pos_w,
            lm_erased=lm_erased, ref_kf=ref_kf, lm_optimized=lm_optimized, pos_after=pos_after))
        set_outputs(a, LOOP_BA_PROPAGATE_OUTPUTS, out, dev_ptr)
        self._device("plp_loop_ba_propagate_device", a, stream)

    def chol_dense(self, A, b, lam=0.0):
        """D23's dense solve (A + lam I) x = b through the panel kernels of plp_global_ba_device (plp_chol_dense_host).  Returns (x, ok)."""
        return _chol_dense(lambda *args: _check(lib().plp_chol_dense_host(self._h, *args)), A, b, lam)

    def local_map(self, kf_covis, kf_parent, kf_children_offsets, kf_children, kf_lm, obs_offsets, obs_kf, frm_lm, k_cap, m_cap, ml_cap=0, kf_erased=None,
                  kf_counts=None, kf_lm_lines=None, kf_kl_counts=None, lm_erased=None, lm_erased_lines=None, LL=None, frm_counts=None, frm_lm_lines=None,
                  frm_kl_counts=None, max_num_local_keyfrms=60, workspace_bytes=0, fcap=None, flcap=None, outputs=None, out=None):
        """module::local_map_updater for B frames over one map snapshot (plp_local_map_host): kf_covis (F, 10), kf_parent (F,),
        kf_children_offsets (F + 1,), kf_children (C,), kf_lm (F, cap), the observation lists obs_offsets (L + 1,), obs_kf (T,), frm_lm (B, stride), all
        i32 with -1 for none; kf_lm_lines (F, lcap) with LL line rows and frm_lm_lines (B, stride) or None; the erased flags u8 and the counts i32 or
        None.  Returns dict(status (B,) u8: LOCAL_MAP_*, num_first, num_kf, nearest_kf, num_lm (B,), local_kf, first_weight (B, k_cap), local_lm, held
        (B, m_cap) and, with lines, num_lines, local_lines, held_lines); `outputs` names the optional ones wanted (default all); out[name]: the caller's
        array (slots the updater does not write keep their values)."""
        return _local_map_host(self._host("plp_local_map_host"), kf_covis, kf_parent, kf_children_offsets, kf_children, kf_lm, obs_offsets, obs_kf, frm_lm,
                               k_cap, m_cap, ml_cap, kf_erased, kf_counts, kf_lm_lines, kf_kl_counts, lm_erased, lm_erased_lines, LL, frm_counts, frm_lm_lines,
                               frm_kl_counts, max_num_local_keyfrms, workspace_bytes, fcap, flcap, outputs, out)

    def local_map_device(self, dims, tables, out, max_num_local_keyfrms=60, workspace_bytes=0, stream=None):
        """plp_local_map_device: dims a dict of the struct's sizes (B, F, C, L, LL, T, cap, lcap, fcap, flcap, k_cap, m_cap, ml_cap and optionally
        frm_stride, frm_stride_lines); tables a dict of LOCAL_MAP_INPUTS and out a dict of LOCAL_MAP_OUTPUTS, each a device pointer (int), a torch
        tensor on the matcher's device or absent / None; asynchronous on the stream"""
        a = _struct(local_map_args_c, dict({k: int(v) for k, v in dims.items()}, max_num_local_keyfrms=int(max_num_local_keyfrms),
                                           workspace_bytes=int(workspace_bytes)), {k: dev_ptr(tables.get(k)) for k in LOCAL_MAP_INPUTS})
        set_outputs(a, LOCAL_MAP_OUTPUTS, out, dev_ptr)
        self._device("plp_local_map_device", a, stream)

    def cull_keyframes(self, kf_lm, undist, kf_id, obs_offsets, obs_kf, obs_idx, cur_kf, covis_offsets, covis, origin_id=0, is_monocular=True,
                       kf_counts=None, x_right=None, depths=None, depth_thr=None, kf_erased=None, kf_cannot_erase=None, lm_erased=None, lm_num_obs=None,
                       outputs=None, out=None):
        """local_map_cleaner::remove_redundant_keyframes for G problems over one map snapshot (plp_cull_keyframes_host):
        kf_lm (F, cap) i32, undist (F, kp_stride) KP_DTYPE, kf_id (F,) u32, the observation lists obs_offsets (L + 1,), obs_kf, obs_idx (T,), cur_kf
        (G,) rows, covis_offsets (G + 1,) into covis (Cv,) rows; x_right / depths (F, kp_stride) f32, depth_thr (F,) f32, the byte tables and lm_num_obs
        (L,) u32 or None.  Returns dict(num_removed (G,), decision (Cv,) u8: CULL_KF_*, num_valid, num_redundant (Cv,), kf_removed (G, F), lm_erased
        (G, L)); `outputs` names the optional ones wanted (default all); out[name]: the caller's array (unwritten slots keep their values)."""
        return _cull_keyframes_host(self._host("plp_cull_keyframes_host"), kf_lm, undist, kf_id, obs_offsets, obs_kf, obs_idx, cur_kf, covis_offsets, covis,
                                    origin_id, is_monocular, kf_counts, x_right, depths, depth_thr, kf_erased, kf_cannot_erase, lm_erased, lm_num_obs, outputs,
                                    out)

    def cull_keyframes_device(self, dims, tables, out, origin_id=0, is_monocular=True, stream=None):
        """plp_cull_keyframes_device: dims a dict of the struct's sizes (F, L, T, cap, G, Cv and optionally kp_stride); tables a dict of
        CULL_KEYFRAMES_INPUTS and out a dict of CULL_KEYFRAMES_OUTPUTS, each a device pointer (int), a torch tensor on the matcher's device or
        absent / None; asynchronous on the stream"""
        a = _struct(cull_keyframes_args_c, dict({k: int(v) for k, v in dims.items()}, origin_id=int(origin_id), is_monocular=int(bool(is_monocular))),
                    {k: dev_ptr(tables.get(k)) for k in CULL_KEYFRAMES_INPUTS})
        set_outputs(a, CULL_KEYFRAMES_OUTPUTS, out, dev_ptr)
        self._device("plp_cull_keyframes_device", a, stream)

    def cull_landmarks(self, fresh_offsets, fresh, num_observed, num_observable, first_kf_id, num_obs, cur_kf_id, num_obs_thr, lm_erased=None,
                       owning_plane=None, out=None):
        """local_map_cleaner::remove_redundant_landmarks[_line] for R fresh lists (plp_cull_landmarks_host; D20): fresh_offsets (R + 1,) into fresh
        (N,) landmark rows; num_observed, num_observable, first_kf_id, num_obs (L,) u32; cur_kf_id, num_obs_thr (R,) u32; lm_erased, owning_plane (L,)
        u8 or None.  Returns dict(state (N,) u8: CULL_HOLD / CULL_DROP / CULL_ERASE, num_removed, num_fresh (R,), fresh (N,): the HOLD entries of
        list r in order from fresh_offsets[r] on)."""
        return _cull_landmarks_host(self._host("plp_cull_landmarks_host"), fresh_offsets, fresh, num_observed, num_observable, first_kf_id, num_obs, cur_kf_id,
                                    num_obs_thr, lm_erased, owning_plane, out)

    def cull_landmarks_device(self, dims, tables, out, stream=None):
        """plp_cull_landmarks_device: dims dict(R, N, L); tables a dict of CULL_LANDMARKS_INPUTS and out a dict of CULL_LANDMARKS_OUTPUTS, device
        pointers (int) or torch tensors; asynchronous, one kernel on the stream"""
        a = _struct(cull_landmarks_args_c, {k: int(v) for k, v in dims.items()}, {k: dev_ptr(tables.get(k)) for k in CULL_LANDMARKS_INPUTS})
        set_outputs(a, CULL_LANDMARKS_OUTPUTS, out, dev_ptr)
        self._device("plp_cull_landmarks_device", a, stream)

    def covisibility_update(self, kf_lm, obs_offsets, obs_kf, kf_id, state, owners, kf_counts=None, lm_erased=None, outputs=None, out=None):
        """graph_node::update_connections of the key frames `owners` (G,), as if one after another in list order, over one map snapshot
        (plp_covisibility_update_host): kf_lm (F, cap) i32, the observation lists obs_offsets (L + 1,), obs_kf (T,), kf_id
        (F,) u32; kf_counts (F,) i32 and lm_erased (L,) u8 or None.  state: a dict of the numpy tables of COVISIBILITY_STATE (covisibility_state()
        makes empty ones), updated in place.  Returns dict(status (G,) u8: COVIS_*, nearest, max_weight (G,), touched (F,) u8); `outputs` names
        the optional ones wanted (default all); out[name]: the caller's array (unwritten slots keep their values).  A list that names a key
        frame twice is refused."""
        return _covisibility_update_host(self._host("plp_covisibility_update_host"), kf_lm, obs_offsets, obs_kf, kf_id, state, owners, kf_counts, lm_erased,
                                         outputs, out)

    def covisibility_update_device(self, dims, tables, out, stream=None):
        """plp_covisibility_update_device: dims a dict of the struct's sizes (F, L, T, cap, conn_cap, covis_cap, G); tables a dict of
        COVISIBILITY_INPUTS and COVISIBILITY_STATE (updated in place) and out a dict of COVISIBILITY_OUTPUTS, each a device pointer (int), a torch
        tensor on the matcher's device or absent / None; asynchronous on the stream"""
        a = _struct(covisibility_update_args_c, {k: int(v) for k, v in dims.items()},
                    {k: dev_ptr(tables.get(k)) for k in COVISIBILITY_INPUTS + tuple(COVISIBILITY_STATE)})
        set_outputs(a, COVISIBILITY_OUTPUTS, out, dev_ptr)
        self._device("plp_covisibility_update_device", a, stream)

    def covisibility_erase(self, state, erased, out=None):
        """graph_node::erase_all_connections of every key frame with erased[k] != 0 (plp_covisibility_erase_host; D21): state as for
        covisibility_update (the six connection tables), erased (F,) u8.  Returns dict(status (F,) u8, touched (F,) u8)."""
        return _covisibility_erase_host(self._host("plp_covisibility_erase_host"), state, erased, out)

    def covisibility_erase_device(self, dims, tables, out, stream=None):
        """plp_covisibility_erase_device: dims dict(F, conn_cap, covis_cap); tables the six connection tables and `erased`, out dict(status,
        touched), device pointers (int) or torch tensors; asynchronous, two launches on the stream"""
        a = _struct(covisibility_erase_args_c, {k: int(v) for k, v in dims.items()},
                    {k: dev_ptr(tables.get(k)) for k in COVISIBILITY_ERASE_STATE + ("erased",)})
        set_outputs(a, ("status", "touched"), out, dev_ptr)
        self._device("plp_covisibility_erase_device", a, stream)

    def bow_query(self, n_words, db_word, db_value, db_n, q_word, q_value, q_n, db_alive=None, reject=None, min_score=None, covis=None, n_covis=None,
                  scoring=0, outputs=None):
        """data::bow_database::acquire_loop_candidates / acquire_relocalization_candidates for Q queries (plp_bow_query_host): db_word (N, stride)
        u32 ascending per row, db_value (N, stride) f64, db_n (N,), db_alive (N,) u8 or None; q_word / q_value (Q, q_stride), q_n (Q,); reject
        (Q, N) u8 or None; min_score (Q,) f32 or None = 0; covis (N, covis_cap) i32 with n_covis (N,), or None.  Returns a dict of the outputs
        named in `outputs` (default: all of BOW_QUERY_OUTPUTS): common, score, total, best_kf, final (Q, N); n_final, max_common, best_total,
        status (Q,)."""
        dw = np.ascontiguousarray(db_word, np.uint32); dv = np.ascontiguousarray(db_value, np.float64)
        qw = np.ascontiguousarray(q_word, np.uint32); qv = np.ascontiguousarray(q_value, np.float64)
        if dw.ndim != 2 or qw.ndim != 2 or dv.shape != dw.shape or qv.shape != qw.shape:
            raise PlpError(PLP_ERR_INVALID_ARG, "db_word / db_value must be (N, stride) and q_word / q_value (Q, q_stride)")
        (N, stride), (Q, q_stride) = dw.shape, qw.shape
        dn = np.ascontiguousarray(db_n, np.int32).reshape(N); qn = np.ascontiguousarray(q_n, np.int32).reshape(Q)
        al = None if db_alive is None else np.ascontiguousarray(db_alive, np.uint8).reshape(N)
        rj = None if reject is None else np.ascontiguousarray(reject, np.uint8).reshape(Q, N)
        ms = None if min_score is None else np.ascontiguousarray(min_score, np.float32).reshape(Q)
        cv = None if covis is None else np.ascontiguousarray(covis, np.int32)
        if cv is not None and (cv.ndim != 2 or cv.shape[0] != N):
            raise PlpError(PLP_ERR_INVALID_ARG, "covis must be (N, covis_cap)")
        nc = None if covis is None else np.ascontiguousarray(n_covis, np.int32).reshape(N)
        o = {k: np.zeros((Q, N) if rows else (Q,), dt) for k, (rows, dt) in BOW_QUERY_OUTPUTS.items() if outputs is None or k in outputs}
        a = _struct(bow_query_args_c, dict(scoring=int(scoring), n_words=int(n_words), N=N, stride=stride, Q=Q, q_stride=q_stride,
                                           covis_cap=0 if cv is None else cv.shape[1]),
                    host_ptrs(db_word=dw, db_value=dv, db_n=dn, db_alive=al, q_word=qw, q_value=qv, q_n=qn, reject=rj, min_score=ms, covis=cv, n_covis=nc))
        set_outputs(a, o, o, host_ptr)
        _check(lib().plp_bow_query_host(self._h, C.byref(a)))
        return o

    def bow_query_device(self, n_words, N, stride, db_word, db_value, db_n, Q, q_stride, q_word, q_value, q_n, out, db_alive=None, reject=None,
                         min_score=None, covis_cap=0, covis=None, n_covis=None, scoring=0, stream=None):
        """plp_bow_query_device: every array a device pointer (int) or a torch tensor on the matcher's device -- min_score too; `out` maps names of
        BOW_QUERY_OUTPUTS to tensors (the others are not written); asynchronous, four kernels on the stream"""
        a = _struct(bow_query_args_c, dict(scoring=int(scoring), n_words=int(n_words), N=int(N), stride=int(stride), Q=int(Q), q_stride=int(q_stride),
                                           covis_cap=int(covis_cap)),
                    dev_ptrs(db_word=db_word, db_value=db_value, db_n=db_n, db_alive=db_alive, q_word=q_word, q_value=q_value, q_n=q_n, reject=reject,
                             min_score=min_score, covis=covis, n_covis=n_covis))
        set_outputs(a, out, out, dev_ptr)
        self._device("plp_bow_query_device", a, stream)

    def bow_score_pairs(self, a_word, a_value, a_n, b_word, b_value, b_n, a_row, b_row, scoring=0):
        """plp_bow_score_pairs_host: (float)score(row a_row[p] of table A, row b_row[p] of table B), (P,) f32; tables as in bow_query"""
        aw = np.ascontiguousarray(a_word, np.uint32); av = np.ascontiguousarray(a_value, np.float64)
        bw = np.ascontiguousarray(b_word, np.uint32); bv = np.ascontiguousarray(b_value, np.float64)
        if aw.ndim != 2 or bw.ndim != 2 or av.shape != aw.shape or bv.shape != bw.shape:
            raise PlpError(PLP_ERR_INVALID_ARG, "the tables must be (rows, stride)")
        an = np.ascontiguousarray(a_n, np.int32).reshape(aw.shape[0]); bn = np.ascontiguousarray(b_n, np.int32).reshape(bw.shape[0])
        ar = np.ascontiguousarray(a_row, np.int32).reshape(-1); br = np.ascontiguousarray(b_row, np.int32).reshape(len(ar))
        out = np.zeros(len(ar), np.float32)
        a = _struct(bow_score_pairs_args_c, dict(scoring=int(scoring), NA=aw.shape[0], stride_a=aw.shape[1], NB=bw.shape[0], stride_b=bw.shape[1], P=len(ar)),
                    host_ptrs(a_word=aw, a_value=av, a_n=an, b_word=bw, b_value=bv, b_n=bn, a_row=ar, b_row=br, out_score=out))
        _check(lib().plp_bow_score_pairs_host(self._h, C.byref(a)))
        return out

    def bow_score_pairs_device(self, NA, stride_a, a_word, a_value, a_n, NB, stride_b, b_word, b_value, b_n, P, a_row, b_row, out_score, scoring=0,
                               stream=None):
        """plp_bow_score_pairs_device: device pointers (int) or torch tensors; asynchronous, one kernel on the stream"""
        a = _struct(bow_score_pairs_args_c, dict(scoring=int(scoring), NA=int(NA), stride_a=int(stride_a), NB=int(NB), stride_b=int(stride_b), P=int(P)),
                    dev_ptrs(a_word=a_word, a_value=a_value, a_n=a_n, b_word=b_word, b_value=b_value, b_n=b_n, a_row=a_row, b_row=b_row, out_score=out_score))
        self._device("plp_bow_score_pairs_device", a, stream)

    def landmark_descriptors_device(self, descs, offsets, L, out_best_idx, stream=None):
        """plp_landmark_descriptor_device: descs [total, 32] u8, offsets [L + 1] i32, out_best_idx [L] i32 on the matcher's device; asynchronous"""
        _check(lib().plp_landmark_descriptor_device(self._h, dev_ptr(descs), dev_ptr(offsets), int(L), dev_ptr(out_best_idx), stream_handle(stream)))

    def lbd_match_1nn(self, query_lbd, train_lbd):
        """BinaryDescriptorMatcher::match: (trainIdx, distance) per query row"""
        q = np.ascontiguousarray(query_lbd, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train_lbd, np.uint8).reshape(-1, 32)
        idx = np.full(len(q), -1, np.int32)
        dist = np.full(len(q), 256, np.int32)
        _check(lib().plp_lbd_match_1nn_host(self._h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist)))
        return idx, dist

    def debug_counters(self):
        v = np.zeros(4, np.int64)
        _check(lib().plp_match_debug_counters(self._h, _p(v)))
        return v

    def hamming_matrix(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        d = np.zeros((len(q), len(t)), np.uint16)
        _check(lib().plp_hamming_matrix_host(self._h, _p(q), len(q), _p(t), len(t), _p(d)))
        return d


# ------------------------------------------------------------------------------------------------
# util::stereo_rectifier of the reference (src/PLPSLAM/util/stereo_rectifier.cc:38-85), perspective model
# ------------------------------------------------------------------------------------------------
class stereo_rectifier:
    """Mirror of util::stereo_rectifier: the constructor takes the rectified camera (fx, fy, cx, cy, cols, rows) and the
    yaml node's StereoRectifier.{K,D,R}_{left,right} lists and builds the two CV_32F map pairs in HBM
    (cv::initUndistortRectifyMap, :61-62); rectify() is the two cv::remap(INTER_LINEAR) calls (:83-84) on batches of 8-bit
    frames.  StereoRectifier.model "perspective" or "fisheye" (cv::fisheye::initUndistortRectifyMap, :67-68); anything else
    raises, like the reference (:72-75, :108)."""

    def __init__(self, camera, yaml_node, device=0):
        import torch
        model = yaml_node.get("StereoRectifier.model", "perspective")
        if model not in ("perspective", "fisheye"):     # "equirectangular" parses in the reference and then throws (:72-75)
            raise PlpError(1, f"Invalid model type for stereo rectification: {model}")
        self.model = model
        self._mt = matcher(device=device)
        self._dev = torch.device("cuda", device)
        self.rows, self.cols = int(camera["rows"]), int(camera["cols"])
        cam = camera_c()
        for k in ("fx", "fy", "cx", "cy"):
            setattr(cam, k, float(camera[k]))
        self.maps = {}
        for eye in ("left", "right"):
            K = np.ascontiguousarray(yaml_node[f"StereoRectifier.K_{eye}"], np.float64)
            D = np.ascontiguousarray(yaml_node[f"StereoRectifier.D_{eye}"], np.float64)
            R = np.ascontiguousarray(yaml_node[f"StereoRectifier.R_{eye}"], np.float64)
            if K.size != 9 or R.size != 9:
                raise PlpError(1, "StereoRectifier.K / R must have 9 entries")
            mx = torch.empty((self.rows, self.cols), dtype=torch.float32, device=self._dev)
            my = torch.empty_like(mx)
            if model == "fisheye":
                if D.size != 4:
                    raise PlpError(1, "the fisheye model takes 4 distortion coefficients")
                _check(lib().plp_rectify_map_fisheye_device(self._mt._h, _p(K), _p(D), _p(R), C.byref(cam), self.rows, self.cols, mx.data_ptr(),
                                                            my.data_ptr(), self.cols * 4, None))
            else:
                _check(lib().plp_rectify_map_device(self._mt._h, _p(K), _p(D) if D.size else None, int(D.size), _p(R), C.byref(cam), self.rows,
                                                    self.cols, mx.data_ptr(), my.data_ptr(), self.cols * 4, None))
            self.maps[eye] = (mx, my)

    def _remap(self, img, eye, stream=None):
        import torch
        if img.dtype != torch.uint8 or img.dim() not in (2, 3) or not img.is_contiguous():
            raise PlpError(1, "rectify expects contiguous uint8 [B,] rows x cols frames on the device")
        B = 1 if img.dim() == 2 else img.shape[0]
        rows, cols = img.shape[-2:]
        out = torch.empty((B, self.rows, self.cols), dtype=torch.uint8, device=img.device)
        mx, my = self.maps[eye]
        st = torch.cuda.current_stream(img.device).cuda_stream if stream is None else stream.cuda_stream
        _check(lib().plp_remap_linear_device(self._mt._h, img.data_ptr(), rows, cols, cols, rows * cols, mx.data_ptr(), my.data_ptr(), self.cols * 4,
                                             self.rows, self.cols, B, out.data_ptr(), self.cols, self.rows * self.cols, st))
        return out[0] if img.dim() == 2 else out

    def rectify(self, in_img_l, in_img_r, stream=None):
        """returns (out_img_l, out_img_r)"""
        return self._remap(in_img_l, "left", stream), self._remap(in_img_r, "right", stream)


# ------------------------------------------------------------------------------------------------
# data::bow_vocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) -- the transform of compute_bow
# ------------------------------------------------------------------------------------------------
class bow_vocabulary:
    """Mirror of data::bow_vocabulary for the one call the front-end makes: transform(descriptors, bow_vec, bow_feat_vec,
    levelsup) (data/frame.cc:785-795).  Built from the node list in m_nodes order: parents[i] (node 0 = root, -1), is_leaf,
    descriptors, weights -- the id rules of DBoW2's loaders (node ids in file order, children appended in file order, word
    ids handed to leaves in file order)."""

    def __init__(self, L, parents, is_leaf, descs, weights, weighting=TF_IDF, scoring=L1_NORM, device=0):
        parents = np.asarray(parents, np.int64); is_leaf = np.asarray(is_leaf, bool)
        n = len(parents)
        descs = np.ascontiguousarray(descs, np.uint8).reshape(n, 32); weights = np.ascontiguousarray(weights, np.float64)
        if n < 2 or parents[0] != -1 or (parents[1:] < 0).any() or (parents[1:] >= np.arange(1, n)).any():
            raise PlpError(1, "node 0 must be the root and every node must follow its parent")
        order = np.argsort(parents[1:], kind="stable") + 1           # children grouped by parent, file order inside a group
        counts = np.bincount(parents[1:], minlength=n)
        if (counts[is_leaf] != 0).any() or (counts[~is_leaf] == 0).any():
            raise PlpError(1, "is_leaf does not agree with the child lists")
        self.child_offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.children = order.astype(np.int32)
        self.node_word = np.zeros(n, np.uint32)
        self.node_word[is_leaf] = np.arange(int(is_leaf.sum()), dtype=np.uint32)
        self.node_desc, self.node_weight, self.L = descs, weights, int(L)
        self.accumulate = 1 if weighting in (TF_IDF, TF) else 0
        self.norm = {L1_NORM: 1, L2_NORM: 2, CHI_SQUARE: 1, KL: 1, BHATTACHARYYA: 1, DOT_PRODUCT: 0}[scoring]
        t = bow_tree_c(n, self.L, _p(self.child_offset), _p(self.children), _p(self.node_desc), _p(self.node_weight), _p(self.node_word),
                       self.accumulate, self.norm)
        h = C.c_void_p()
        _check(lib().plp_bow_vocab_create(device, C.byref(t), C.byref(h)))
        self._h = h
        self.device = device

    @staticmethod
    def parse_text_file(path):
        """ORB-SLAM2-style ORBvoc.txt (DBoW2 TemplatedVocabulary::loadFromTextFile): 'k L scoring weighting', then one line per
        node 'parent is_leaf d0 .. d31 weight'.  Host only.  Returns (L, parents, is_leaf, descs, weights, weighting, scoring)."""
        with open(path) as f:
            head = f.readline().split()
            if len(head) != 4:
                raise PlpError(1, "vocabulary header must be 'k L scoring weighting'")
            k, L, scoring, weighting = (int(v) for v in head)
            if not (0 <= k <= 20 and 1 <= L <= 10 and 0 <= scoring <= 5 and 0 <= weighting <= 3):
                raise PlpError(1, "vocabulary parameters out of range")      # the same sanity check loadFromTextFile makes
            rows = [ln.split() for ln in f if ln.strip()]
        if any(len(r) != 35 for r in rows):
            raise PlpError(1, "a node line must hold parent, is_leaf, 32 descriptor bytes and the weight")
        parents = [-1] + [int(r[0]) for r in rows]
        leaf = [False] + [int(r[1]) > 0 for r in rows]
        descs = np.zeros((len(rows) + 1, 32), np.uint8)
        if rows:
            descs[1:] = np.array([[int(v) for v in r[2:34]] for r in rows], np.uint8)
        weights = [0.0] + [float(r[34]) for r in rows]
        return L, parents, leaf, descs, weights, weighting, scoring

    @classmethod
    def from_text_file(cls, path, device=0):
        L, parents, leaf, descs, weights, weighting, scoring = cls.parse_text_file(path)
        return cls(L, parents, leaf, descs, weights, weighting, scoring, device)

    # ---- binary vocabulary (`orb_vocab.dbow2`, README.md:147 of the reference; system.cc loads it with loadFromBinaryFile)
    # DBoW2 itself and the blob are not in the reference tree: the layout below is the published one of the binary-vocabulary
    # patch that OpenVSLAM's DBoW2 fork carries (TemplatedVocabulary::saveToBinaryFile / loadFromBinaryFile), parity unpinned:
    #   u32 nb_nodes (= m_nodes.size(), root included)   u32 size_node (= 4 + 32 + 4 + 1)   i32 k   i32 L   i32 scoring   i32 weighting
    #   then, for node ids 1 .. nb_nodes-1 in order:  i32 parent | 32 descriptor bytes | f32 weight | u8 is_leaf
    _DBOW2_NODE = np.dtype([("parent", "<i4"), ("desc", "u1", (32,)), ("weight", "<f4"), ("leaf", "u1")])

    @staticmethod
    def parse_dbow2_file(path, replicate_eof_node=True):
        """Host only.  Returns (L, parents, is_leaf, descs, weights, weighting, scoring) like parse_text_file.
        replicate_eof_node: the loader reads records `while (!f.eof())`, so after the last record one more iteration runs on the
        stale buffer and appends a copy of the last node (same parent, same descriptor; a new word id if it is a leaf) -- which is
        why it sizes m_nodes to nb_nodes + 1.  The copy can never win a descent (first minimum wins) but it is part of what the
        reference holds in memory, so it is reproduced by default."""
        raw = np.fromfile(path, np.uint8)
        if raw.size < 24:
            raise PlpError(1, "vocabulary file shorter than its header")
        nb_nodes, size_node = (int(v) for v in raw[:8].view("<u4"))
        k, L, scoring, weighting = (int(v) for v in raw[8:24].view("<i4"))
        if size_node != bow_vocabulary._DBOW2_NODE.itemsize:
            raise PlpError(1, f"node records of {size_node} bytes: not a 256-bit ORB vocabulary")
        if not (0 <= k <= 20 and 1 <= L <= 10 and 0 <= scoring <= 5 and 0 <= weighting <= 3):
            raise PlpError(1, "vocabulary parameters out of range")
        body = raw[24:]
        n_rec = body.size // size_node
        if n_rec != nb_nodes - 1:
            raise PlpError(1, f"{n_rec} node records for nb_nodes = {nb_nodes}")
        rec = body[:n_rec * size_node].view(bow_vocabulary._DBOW2_NODE)
        if replicate_eof_node and n_rec:
            rec = np.concatenate([rec, rec[-1:]])
        parents = np.concatenate([[-1], rec["parent"].astype(np.int64)])
        leaf = np.concatenate([[False], rec["leaf"] != 0])
        descs = np.concatenate([np.zeros((1, 32), np.uint8), rec["desc"]])
        weights = np.concatenate([[0.0], rec["weight"].astype(np.float64)])
        return L, parents, leaf, descs, weights, weighting, scoring

    @staticmethod
    def write_dbow2_file(path, k, L, parents, is_leaf, descs, weights, weighting=TF_IDF, scoring=L1_NORM):
        """saveToBinaryFile's layout (node 0 = root is not written); for tests and for converting a text vocabulary"""
        n = len(parents)
        rec = np.zeros(n - 1, bow_vocabulary._DBOW2_NODE)
        rec["parent"] = np.asarray(parents[1:], np.int32); rec["desc"] = np.asarray(descs, np.uint8).reshape(n, 32)[1:]
        rec["weight"] = np.asarray(weights[1:], np.float32); rec["leaf"] = np.asarray(is_leaf[1:], bool)
        with open(path, "wb") as f:
            f.write(np.array([n, rec.dtype.itemsize], "<u4").tobytes())
            f.write(np.array([k, L, scoring, weighting], "<i4").tobytes())
            f.write(rec.tobytes())

    @classmethod
    def from_dbow2_file(cls, path, device=0, replicate_eof_node=True):
        L, parents, leaf, descs, weights, weighting, scoring = cls.parse_dbow2_file(path, replicate_eof_node)
        return cls(L, parents, leaf, descs, weights, weighting, scoring, device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().plp_bow_vocab_destroy(h)
            self._h = None

    def transform_device(self, desc, counts=None, levelsup=4, stream=None):
        """desc: uint8 [B, cap, 32] on the device.  Returns a dict of device tensors:
        word_id, node_id [B, cap]; bow_word, bow_value, n_bow; fv_node, fv_feat, n_fv."""
        import torch
        B, cap = desc.shape[0], desc.shape[1]
        dev = desc.device
        o = dict(word_id=torch.empty((B, cap), dtype=torch.int32, device=dev), node_id=torch.empty((B, cap), dtype=torch.int32, device=dev),
                 bow_word=torch.empty((B, cap), dtype=torch.int32, device=dev), bow_value=torch.empty((B, cap), dtype=torch.float64, device=dev),
                 n_bow=torch.empty(B, dtype=torch.int32, device=dev), fv_node=torch.empty((B, cap), dtype=torch.int32, device=dev),
                 fv_feat=torch.empty((B, cap), dtype=torch.int32, device=dev), n_fv=torch.empty(B, dtype=torch.int32, device=dev))
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
        _check(lib().plp_bow_transform_device(self._h, desc.data_ptr(), counts.data_ptr() if counts is not None else None, cap, B, levelsup,
                                              o["word_id"].data_ptr(), o["node_id"].data_ptr(), o["bow_word"].data_ptr(), o["bow_value"].data_ptr(),
                                              o["n_bow"].data_ptr(), o["fv_node"].data_ptr(), o["fv_feat"].data_ptr(), o["n_fv"].data_ptr(), st))
        return o

    def transform(self, desc, levelsup=4):
        """one frame, numpy in / out: (bow_vec {word: value}, bow_feat_vec {node: [features]}, word_id, node_id)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        word = np.zeros(max(n, 1), np.uint32); node = np.zeros(max(n, 1), np.uint32)
        bw = np.zeros(max(n, 1), np.uint32); bv = np.zeros(max(n, 1), np.float64); fn = np.zeros(max(n, 1), np.uint32); ff = np.zeros(max(n, 1), np.uint32)
        nb, nf = C.c_int32(), C.c_int32()
        _check(lib().plp_bow_transform_host(self._h, _p(desc) if n else None, n, levelsup, _p(word), _p(node), _p(bw), _p(bv), C.byref(nb), _p(fn), _p(ff),
                                            C.byref(nf)))
        bow_vec = dict(zip(bw[:nb.value].tolist(), bv[:nb.value].tolist()))
        feat_vec = {}
        for nd, fi in zip(fn[:nf.value].tolist(), ff[:nf.value].tolist()):
            feat_vec.setdefault(nd, []).append(fi)
        return bow_vec, feat_vec, word[:n].copy(), node[:n].copy()


# ------------------------------------------------------------------------------------------------
class bow_database:
    """Mirror of data::bow_database (src/PLPSLAM/data/bow_database.cc) on the device: a table of BowVectors, one row per key frame, in the layout
    bow_vocabulary.transform_device writes, and the two candidate queries over it (plp_bow_query_device).  The caller binds key-frame ids to rows
    (INTEGRATION.md section 3).  The score is DBoW2's L1 score restated from the published algorithm: parity unpinned.

    n_words: an upper bound of every word id (the vocabulary's word count); stride: slots of a row (the cap of the transform, or tighter);
    covis_cap: slots of a covisibility row (get_top_n_covisibilities(10) -> 10).  The tables grow by doubling."""

    def __init__(self, n_words, stride, covis_cap=10, scoring=L1_NORM, capacity=64, device=0):
        import torch
        if scoring != L1_NORM:
            raise PlpError(PLP_ERR_UNSUPPORTED, "only L1_NORM scoring is implemented")
        if not (1 <= stride <= 8192 and 0 <= covis_cap <= 16 and n_words > 0):
            raise PlpError(PLP_ERR_INVALID_ARG, "stride must be 1 .. 8192, covis_cap 0 .. 16, n_words positive")
        self.torch, self.dev, self.device = torch, torch.device("cuda", device), device
        self.n_words, self.stride, self.covis_cap, self.scoring = int(n_words), int(stride), int(covis_cap), int(scoring)
        self.N = 0                                 # rows in use: 1 + the highest row ever added
        self.mt = matcher(device=device)
        self._alloc(max(int(capacity), 1))

    def _alloc(self, cap):
        torch = self.torch
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        new = dict(word=z((cap, self.stride), torch.int32), value=z((cap, self.stride), torch.float64), n=z((cap,), torch.int32),
                   alive=z((cap,), torch.uint8), covis=z((cap, max(self.covis_cap, 1)), torch.int32), n_covis=z((cap,), torch.int32))
        old = getattr(self, "t", None)
        if old is not None:
            for k, v in old.items():
                new[k][:v.shape[0]].copy_(v)
        self.t, self.capacity = new, cap

    def _stream(self, stream):
        return stream or self.torch.cuda.current_stream(self.dev)

    def add_keyframe(self, row, bow_word, bow_value, n_bow, stream=None):
        """bow_database::add_keyframe (:24-40): row <- one BowVector.  bow_word / bow_value: 1-D device tensors (a row of transform_device's
        bow_word / bow_value; the first min(len, stride) slots are copied), n_bow: its count, a device tensor of one element or an int, of which at
        most `stride` are used.  Device copies on the stream."""
        torch = self.torch
        row = int(row)
        with torch.cuda.stream(self._stream(stream)):
            if row >= self.capacity:
                cap = self.capacity
                while cap <= row:
                    cap *= 2
                self._alloc(cap)
            m = min(int(bow_word.shape[0]), self.stride)
            self.t["word"][row, :m].copy_(bow_word[:m].view(torch.int32) if bow_word.dtype != torch.int32 else bow_word[:m])
            self.t["value"][row, :m].copy_(bow_value[:m])
            if isinstance(n_bow, int):
                self.t["n"][row:row + 1].fill_(min(n_bow, m))
            else:
                self.t["n"][row:row + 1].copy_(n_bow.reshape(1).clamp(max=m))
            self.t["alive"][row:row + 1].fill_(1)
        self.N = max(self.N, row + 1)

    def erase_keyframe(self, row, stream=None):
        """bow_database::erase_keyframe (:42-66): the row shares no word with anything from now on"""
        if 0 <= int(row) < self.N:
            with self.torch.cuda.stream(self._stream(stream)):
                self.t["alive"][int(row):int(row) + 1].fill_(0)

    def clear(self, stream=None):
        """bow_database::clear (:68-77)"""
        with self.torch.cuda.stream(self._stream(stream)):
            self.t["alive"].zero_()
            self.t["n_covis"].zero_()
        self.N = 0

    def set_covisibilities(self, row, rows, stream=None):
        """the key frame's get_top_n_covisibilities(10), as database rows in that order: a list of ints or a device i32 tensor"""
        torch = self.torch
        row, n = int(row), len(rows)
        if not (0 <= row < self.capacity) or n > self.covis_cap:
            raise PlpError(PLP_ERR_INVALID_ARG, "row outside the table or more than covis_cap covisibilities")
        with torch.cuda.stream(self._stream(stream)):
            if n:
                src = rows if isinstance(rows, torch.Tensor) else torch.tensor([int(r) for r in rows], dtype=torch.int32).to(self.dev)
                self.t["covis"][row, :n].copy_(src)
            self.t["n_covis"][row:row + 1].fill_(n)

    def _query_device(self, q_word, q_value, q_n, min_score, reject, stream, outputs):
        torch = self.torch
        if q_word.dim() == 1:
            q_word, q_value, q_n = q_word.unsqueeze(0), q_value.unsqueeze(0), q_n.reshape(1)
        Q, qs = q_word.shape
        if not (q_word.is_contiguous() and q_value.is_contiguous()):
            raise PlpError(PLP_ERR_INVALID_ARG, "q_word and q_value must be contiguous (Q, q_stride) tensors")
        st = self._stream(stream)
        tt = {np.uint32: torch.int32, np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}
        with torch.cuda.stream(st):
            out = {k: torch.empty((Q, self.N) if rows else (Q,), dtype=tt[dt], device=self.dev) for k, (rows, dt) in BOW_QUERY_OUTPUTS.items()
                   if outputs is None or k in outputs}
        t = self.t
        self.mt.bow_query_device(self.n_words, self.N, self.stride, t["word"], t["value"], t["n"], Q, qs, q_word, q_value, q_n, out, db_alive=t["alive"],
                                 reject=reject, min_score=min_score, covis_cap=self.covis_cap, covis=t["covis"] if self.covis_cap else None,
                                 n_covis=t["n_covis"] if self.covis_cap else None, scoring=self.scoring, stream=st)
        return out

    def acquire_loop_candidates_device(self, q_word, q_value, q_n, min_score, reject=None, stream=None, outputs=None):
        """bow_database::acquire_loop_candidates (:97-168) for Q query key frames: q_word / q_value (Q, q_stride) and q_n (Q,) device tensors (or one
        query, 1-D), min_score (Q,) f32 DEVICE tensor (score_pairs_device -> torch minimum: it never visits the host), reject (Q, N) u8 device tensor
        -- the query's connected key frames and the query itself -- or None.  Returns the device tensors of BOW_QUERY_OUTPUTS (u32 as i32);
        `final` is the candidate mask over the rows.  Asynchronous."""
        if reject is not None and tuple(reject.shape)[-1] != self.N:
            raise PlpError(PLP_ERR_INVALID_ARG, "reject must be (Q, N) for the N rows in use")
        return self._query_device(q_word, q_value, q_n, min_score, reject, stream, outputs)

    def acquire_relocalization_candidates_device(self, q_word, q_value, q_n, stream=None, outputs=None):
        """bow_database::acquire_relocalization_candidates (:170-236): no rejected key frames, min_score 0"""
        return self._query_device(q_word, q_value, q_n, None, None, stream, outputs)

    def _rows(self, out, single):
        self.torch.cuda.current_stream(self.dev).synchronize()
        final = out["final"].cpu().numpy()
        lists = [np.flatnonzero(f).tolist() for f in final]
        return lists[0] if single else lists

    def acquire_loop_candidates(self, q_word, q_value, q_n, min_score, reject=None):
        """host form: the sorted list of candidate rows (a list per query for 2-D queries); min_score a float, a sequence or a device tensor"""
        torch = self.torch
        single = q_word.dim() == 1
        if not isinstance(min_score, torch.Tensor):
            min_score = torch.tensor(np.asarray(min_score, np.float32).reshape(-1)).to(self.dev)
        return self._rows(self.acquire_loop_candidates_device(q_word, q_value, q_n, min_score, reject, outputs=("final",)), single)

    def acquire_relocalization_candidates(self, q_word, q_value, q_n):
        return self._rows(self.acquire_relocalization_candidates_device(q_word, q_value, q_n, outputs=("final",)), q_word.dim() == 1)

    def score_pairs_device(self, a_rows, b_rows, stream=None):
        """(float)bow_vocab_->score(row a, row b) for device i32 tensors of rows of this database: (P,) f32 device tensor.  The minimum of these over
        a key frame's covisibilities and 1.0f is loop_detector::compute_min_score_in_covisibilities (module/loop_detector.cc:238-266)."""
        torch = self.torch
        P = int(a_rows.shape[0])
        st = self._stream(stream)
        with torch.cuda.stream(st):
            out = torch.empty((P,), dtype=torch.float32, device=self.dev)
        t = self.t
        self.mt.bow_score_pairs_device(self.N, self.stride, t["word"], t["value"], t["n"], self.N, self.stride, t["word"], t["value"], t["n"], P, a_rows,
                                       b_rows, out, scoring=self.scoring, stream=st)
        return out

    def score(self, a, b):
        """bow_vocab_->score(bow_vec of row a, bow_vec of row b) as the float the reference keeps"""
        torch = self.torch
        rows = torch.tensor([[int(a)], [int(b)]], dtype=torch.int32).to(self.dev)
        return float(self.score_pairs_device(rows[0], rows[1]).cpu()[0])
