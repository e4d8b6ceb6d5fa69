"""The line map update every optimiser ends with (include/plp_front.h: plp_trim_line_endpoints_*, plp_correct_landmark_lines_*,
plp_loop_ba_propagate_lines_*, the plp_model_* host builds): the struct mirrors and status codes, the numpy side of the
host-pointer entries and host builds, and the matcher's methods."""

import ctypes as C

import numpy as np

from ._abi import KL_DTYPE, _struct, camera_model_c
from ._core import PLP_ERR_INVALID_ARG, PlpError
from ._marshal import array_or_none, dev_ptrs, host_ptr, host_ptrs, model_call, out_arrays, set_outputs

_VP = C.c_void_p


class trim_line_endpoints_args_c(C.Structure):
    """plp_trim_line_endpoints_args"""
    _fields_ = [("camera", camera_model_c), ("mode", C.c_int32), ("max_change", C.c_double)] + [(k, C.c_int32) for k in ("L", "F", "cap", "pose_stride")] + [
        (k, _VP) for k in ("pluecker", "ref_kf", "skip", "obs_offsets", "obs_kf", "obs_idx", "pose", "kf_erased", "keylines", "counts", "pos_w_old", "median_depth",
                           "out_pos_w", "out_status", "out_erase")]


class correct_landmark_lines_args_c(C.Structure):
    """plp_correct_landmark_lines_args"""
    _fields_ = [("L", C.c_int32), ("F", C.c_int32)] + [(k, _VP) for k in ("pluecker", "lm_erased", "ref_kf", "corr_kf", "kf_erased", "sim3_cw", "corrected_wc",
                                                                         "out_pluecker", "out_status")]


class loop_ba_propagate_lines_args_c(C.Structure):
    """plp_loop_ba_propagate_lines_args"""
    _fields_ = [("L", C.c_int32), ("F", C.c_int32)] + [(k, _VP) for k in ("pose_after", "pose_before", "kf_status", "pluecker", "lm_erased", "ref_kf", "line_optimized",
                                                                         "pluecker_after", "out_pluecker", "out_status")]


# plp_trim_mode / plp_trim_status / plp_correct_line_status (plp_loop_ba_propagate_lines_* writes LOOP_BA_LM_*)
TRIM_DEPTH_POSITIVE, TRIM_MAX_CHANGE = range(2)
TRIM_OK, TRIM_SKIPPED, TRIM_NO_REF, TRIM_NOT_OBSERVED, TRIM_INDEX_RANGE, TRIM_REJECTED = range(6)
CORRECT_LINE_OK, CORRECT_LINE_ERASED, CORRECT_LINE_NO_REF, CORRECT_LINE_NO_VERTEX = range(4)
TRIM_MAX_CHANGE_THR = 0.1               # local_bundle_adjuster_extended_line.cc:777

# the outputs: name -> (row shape, dtype)
TRIM_OUTPUTS = dict(pos_w=((6,), np.float64), status=((), np.uint8), erase=((), np.uint8))
LINE_MOVE_OUTPUTS = dict(pluecker=((6,), np.float64), status=((), np.uint8))


def _outputs(spec, L, out):
    return out_arrays(((k, (L,) + shape, dt) for k, (shape, dt) in spec.items()), out)


def _trim_fields(camera, mode, max_change, L, F, cap, pose_stride):
    a = trim_line_endpoints_args_c()
    a.camera = camera_model_c.from_buffer_copy(camera)
    a.mode, a.max_change, a.L, a.F, a.cap, a.pose_stride = int(mode), float(max_change), int(L), int(F), int(cap), int(pose_stride)
    return a


def _trim_line_endpoints_host(call, camera, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx, pose, keylines, mode, skip, kf_erased, counts, pos_w_old, median_depth,
                              max_change, out):
    """the numpy side of plp_trim_line_endpoints_host and plp_model_trim_line_endpoints_host: call(args struct) runs the entry"""
    pk = np.ascontiguousarray(pluecker, np.float64).reshape(-1, 6)
    L = len(pk)
    po = np.ascontiguousarray(pose, np.float64)
    if po.ndim != 2 or (po.shape[0] and po.shape[1] < 12):
        raise PlpError(PLP_ERR_INVALID_ARG, "pose must be (F, pose_stride >= 12)")
    F = po.shape[0]
    kl = np.ascontiguousarray(keylines, KL_DTYPE)
    kl = kl.reshape(F, -1) if F else kl.reshape(0, 0)
    rk = np.ascontiguousarray(ref_kf, np.int32).reshape(L)
    oo, ok, oi = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (obs_offsets, obs_kf, obs_idx))
    if len(oo) != L + 1 or len(ok) != len(oi) or (L and int(oo[-1]) > len(ok)):
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_offsets must have L + 1 entries and end inside obs_kf / obs_idx, which have one length")
    sk, ke, cn = array_or_none(skip, np.uint8, L), array_or_none(kf_erased, np.uint8, F), array_or_none(counts, np.int32, F)
    o = _outputs(TRIM_OUTPUTS, L, out)
    # pos_w_old may be the array given as out["pos_w"]: the entry then reads and writes one array
    old = o["pos_w"] if pos_w_old is not None and pos_w_old is o["pos_w"] else array_or_none(pos_w_old, np.float64, L, 6)
    md = array_or_none(median_depth, np.float32, F)
    a = _trim_fields(camera, mode, max_change, L, F, kl.shape[1], po.shape[1] if F else 12)
    for k, v in host_ptrs(pluecker=pk, ref_kf=rk, skip=sk, obs_offsets=oo, obs_kf=ok, obs_idx=oi, pose=po, kf_erased=ke, keylines=kl, counts=cn, pos_w_old=old,
                          median_depth=md).items():
        setattr(a, k, v)
    set_outputs(a, TRIM_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_trim_line_endpoints(camera, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx, pose, keylines, mode=TRIM_DEPTH_POSITIVE, skip=None, kf_erased=None, counts=None,
                              pos_w_old=None, median_depth=None, max_change=TRIM_MAX_CHANGE_THR, out=None):
    """Host build of endpoint_trimming and its call sites' array half (csrc/line_update.hpp; no GPU needed): the arguments and the
    result of matcher.trim_line_endpoints."""
    return _trim_line_endpoints_host(model_call("plp_model_trim_line_endpoints_host", "L", neg_status=True), camera, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx,
                                     pose, keylines, mode, skip, kf_erased, counts, pos_w_old, median_depth, max_change, out)


def _correct_landmark_lines_host(call, pluecker, ref_kf, sim3_cw, corrected_wc, corr_kf, lm_erased, kf_erased, out):
    pk = np.ascontiguousarray(pluecker, np.float64).reshape(-1, 6)
    L = len(pk)
    cw, wc = np.ascontiguousarray(sim3_cw, np.float64).reshape(-1, 8), np.ascontiguousarray(corrected_wc, np.float64).reshape(-1, 8)
    F = len(cw)
    if len(wc) != F:
        raise PlpError(PLP_ERR_INVALID_ARG, "sim3_cw and corrected_wc must both be (F, 8)")
    rk, ck = np.ascontiguousarray(ref_kf, np.int32).reshape(L), array_or_none(corr_kf, np.int32, L)
    le, ke = array_or_none(lm_erased, np.uint8, L), array_or_none(kf_erased, np.uint8, F)
    o = _outputs(LINE_MOVE_OUTPUTS, L, out)
    a = _struct(correct_landmark_lines_args_c, dict(L=L, F=F), host_ptrs(pluecker=pk, lm_erased=le, ref_kf=rk, corr_kf=ck, kf_erased=ke, sim3_cw=cw, corrected_wc=wc))
    set_outputs(a, LINE_MOVE_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_correct_landmark_lines(pluecker, ref_kf, sim3_cw, corrected_wc, corr_kf=None, lm_erased=None, kf_erased=None, out=None):
    """Host build of the line cloud of graph_optimizer::optimize (:352-403; no GPU needed): the arguments and the result of matcher.correct_landmark_lines"""
    return _correct_landmark_lines_host(model_call("plp_model_correct_landmark_lines_host", "L", neg_status=True), pluecker, ref_kf, sim3_cw, corrected_wc, corr_kf,
                                        lm_erased, kf_erased, out)


def _loop_ba_propagate_lines_host(call, pose_after, pose_before, kf_status, pluecker, ref_kf, line_optimized, pluecker_after, lm_erased, out):
    pk = np.ascontiguousarray(pluecker, np.float64).reshape(-1, 6)
    L = len(pk)
    pa, pb = np.ascontiguousarray(pose_after, np.float64).reshape(-1, 15), np.ascontiguousarray(pose_before, np.float64).reshape(-1, 12)
    F = len(pa)
    if len(pb) != F:
        raise PlpError(PLP_ERR_INVALID_ARG, "pose_after must be (F, 15) and pose_before (F, 12)")
    ks, rk = np.ascontiguousarray(kf_status, np.uint8).reshape(F), np.ascontiguousarray(ref_kf, np.int32).reshape(L)
    lo, pq, le = array_or_none(line_optimized, np.uint8, L), array_or_none(pluecker_after, np.float64, L, 6), array_or_none(lm_erased, np.uint8, L)
    o = _outputs(LINE_MOVE_OUTPUTS, L, out)
    a = _struct(loop_ba_propagate_lines_args_c, dict(L=L, F=F), host_ptrs(pose_after=pa, pose_before=pb, kf_status=ks, pluecker=pk, lm_erased=le, ref_kf=rk,
                                                                           line_optimized=lo, pluecker_after=pq))
    set_outputs(a, LINE_MOVE_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_loop_ba_propagate_lines(pose_after, pose_before, kf_status, pluecker, ref_kf, line_optimized=None, pluecker_after=None, lm_erased=None, out=None):
    """Host build of the line cloud of loop_bundle_adjuster::optimize (:184-244; no GPU needed): the arguments and the result of
    matcher.loop_ba_propagate_lines"""
    return _loop_ba_propagate_lines_host(model_call("plp_model_loop_ba_propagate_lines_host", "L", neg_status=True), pose_after, pose_before, kf_status, pluecker,
                                         ref_kf, line_optimized, pluecker_after, lm_erased, out)


class line_update_entries:
    """The matcher's line map update (a base of plp.matcher)."""

    def trim_line_endpoints(self, camera, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx, pose, keylines, mode=TRIM_DEPTH_POSITIVE, skip=None, kf_erased=None,
                            counts=None, pos_w_old=None, median_depth=None, max_change=TRIM_MAX_CHANGE_THR, out=None):
        """endpoint_trimming for L lines over F key frames and what its call sites do with the result (plp_trim_line_endpoints_host):
        pluecker (L, 6) = (m, d), ref_kf (L,), the observation lists as matcher.landmark_line_geometry takes them, pose (F, >= 12) the CURRENT poses, keylines
        (F, cap) KL_DTYPE; mode TRIM_DEPTH_POSITIVE (graph, loop and global adjusters) or TRIM_MAX_CHANGE (the local adjuster: pos_w_old (L, 6), median_depth (F,)
        f32).  Returns dict(pos_w (L, 6): written where status is TRIM_OK, status (L,) u8: TRIM_*, erase (L,) u8); out: arrays to write into, whose other
        slots keep their values -- out["pos_w"] may be pos_w_old itself."""
        return _trim_line_endpoints_host(self._host("plp_trim_line_endpoints_host"), camera, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx, pose, keylines, mode, skip,
                                         kf_erased, counts, pos_w_old, median_depth, max_change, out)

    def trim_line_endpoints_device(self, camera, L, F, cap, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx, pose, keylines, out_pos_w, out_status, out_erase,
                                   mode=TRIM_DEPTH_POSITIVE, skip=None, kf_erased=None, counts=None, pos_w_old=None, median_depth=None,
                                   max_change=TRIM_MAX_CHANGE_THR, pose_stride=15, stream=None):
        """plp_trim_line_endpoints_device: device pointers (int) or torch tensors; out_pos_w may be pos_w_old; asynchronous"""
        a = _trim_fields(camera, mode, max_change, L, F, cap, pose_stride)
        for k, v in dev_ptrs(pluecker=pluecker, ref_kf=ref_kf, skip=skip, obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx, pose=pose, kf_erased=kf_erased,
                             keylines=keylines, counts=counts, pos_w_old=pos_w_old, median_depth=median_depth, out_pos_w=out_pos_w, out_status=out_status,
                             out_erase=out_erase).items():
            setattr(a, k, v)
        self._device("plp_trim_line_endpoints_device", a, stream)

    def correct_landmark_lines(self, pluecker, ref_kf, sim3_cw, corrected_wc, corr_kf=None, lm_erased=None, kf_erased=None, out=None):
        """The line cloud of graph_optimizer::optimize (:352-403; plp_correct_landmark_lines_host): pluecker (L, 6), ref_kf (L,) the row that is tested, corr_kf
        (L,) the row each line is corrected with (None = ref_kf), sim3_cw / corrected_wc (F, 8) of one problem.  Returns dict(pluecker (L, 6): written where status
        is CORRECT_LINE_OK, status (L,) u8)."""
        return _correct_landmark_lines_host(self._host("plp_correct_landmark_lines_host"), pluecker, ref_kf, sim3_cw, corrected_wc, corr_kf, lm_erased, kf_erased, out)

    def correct_landmark_lines_device(self, L, F, pluecker, ref_kf, sim3_cw, corrected_wc, out_pluecker, out_status, corr_kf=None, lm_erased=None, kf_erased=None,
                                      stream=None):
        """plp_correct_landmark_lines_device: device pointers (int) or torch tensors; out_pluecker may be pluecker; asynchronous"""
        a = _struct(correct_landmark_lines_args_c, dict(L=int(L), F=int(F)), dev_ptrs(
            pluecker=pluecker, lm_erased=lm_erased, ref_kf=ref_kf, corr_kf=corr_kf, kf_erased=kf_erased, sim3_cw=sim3_cw, corrected_wc=corrected_wc,
            out_pluecker=out_pluecker, out_status=out_status))
        self._device("plp_correct_landmark_lines_device", a, stream)

    def loop_ba_propagate_lines(self, pose_after, pose_before, kf_status, pluecker, ref_kf, line_optimized=None, pluecker_after=None, lm_erased=None, out=None):
        """The line cloud of loop_bundle_adjuster::optimize (:184-244; plp_loop_ba_propagate_lines_host) over the pose (F, 15), pose_before (F, 12) and kf_status
        (F,) matcher.loop_ba_propagate returned.  Returns dict(pluecker (L, 6): written for LOOP_BA_LM_OPTIMIZED and LOOP_BA_LM_MOVED rows, status (L,) u8)."""
        return _loop_ba_propagate_lines_host(self._host("plp_loop_ba_propagate_lines_host"), pose_after, pose_before, kf_status, pluecker, ref_kf, line_optimized,
                                             pluecker_after, lm_erased, out)

    def loop_ba_propagate_lines_device(self, L, F, pose_after, pose_before, kf_status, pluecker, ref_kf, out_pluecker, out_status, line_optimized=None,
                                       pluecker_after=None, lm_erased=None, stream=None):
        """plp_loop_ba_propagate_lines_device: device pointers (int) or torch tensors; out_pluecker may be pluecker; asynchronous"""
        a = _struct(loop_ba_propagate_lines_args_c, dict(L=int(L), F=int(F)), dev_ptrs(
            pose_after=pose_after, pose_before=pose_before, kf_status=kf_status, pluecker=pluecker, lm_erased=lm_erased, ref_kf=ref_kf, line_optimized=line_optimized,
            pluecker_after=pluecker_after, out_pluecker=out_pluecker, out_status=out_status))
        self._device("plp_loop_ba_propagate_lines_device", a, stream)
