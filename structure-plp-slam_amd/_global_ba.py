"""Global bundle adjustment and the loop adjuster's map update (include/plp_front.h: plp_global_ba_*, plp_loop_ba_propagate_*, the plp_model_* host
builds): the numpy side of the host-pointer entries and host builds, and the mirror classes under the reference's names."""

import ctypes as C

import numpy as np

from ._abi import KP_DTYPE, _struct, camera_model_c, global_ba_args_c, loop_ba_propagate_args_c
from ._core import PLP_ERR_INVALID_ARG, PlpError, _check, lib
from ._marshal import array_or_none, host_ptr, host_ptrs, model_call, out_arrays, set_outputs, wanted

# the outputs of plp_global_ba_*: name -> (shape given (F, L, T), dtype, optional); info[3] is a POSE_OPT_END_* (0: not run)
GLOBAL_BA_OUTPUTS = dict(status=(lambda F, L, T: (1,), np.uint8, False), kf_optimized=(lambda F, L, T: (F,), np.uint8, False),
                         lm_optimized=(lambda F, L, T: (L,), np.uint8, False), pose=(lambda F, L, T: (F, 15), np.float64, False),
                         pos_w=(lambda F, L, T: (L, 3), np.float64, False), info=(lambda F, L, T: (4,), np.int32, True), chi2=(lambda F, L, T: (3,), np.float64, True))
# the outputs of plp_loop_ba_propagate_*: name -> (shape given (F, L), dtype)
LOOP_BA_PROPAGATE_OUTPUTS = dict(pose=(lambda F, L: (F, 15), np.float64), pose_before=(lambda F, L: (F, 12), np.float64), kf_status=(lambda F, L: (F,), np.uint8),
                                 pos_w=(lambda F, L: (L, 3), np.float64), lm_status=(lambda F, L: (L,), np.uint8))


def _global_ba_inputs(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin, lm_erased,
                      num_iter, use_huber_kernel, stop):
    """the input half of a plp_global_ba_args from numpy arrays: (args struct, the arrays it points to, F, L, T)"""
    po = np.ascontiguousarray(pose, np.float64)
    if po.ndim != 2 or po.shape[1] < 12:
        raise PlpError(PLP_ERR_INVALID_ARG, "pose must be (F, pose_stride >= 12)")
    F = po.shape[0]
    ku = np.ascontiguousarray(undist, KP_DTYPE)
    ku = ku.reshape(F, -1) if F else ku.reshape(0, 0)
    K = ku.shape[1]
    xr = array_or_none(x_right, np.float32, F, K)
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    L = len(pw)
    oo, ok, oi = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (obs_offsets, obs_kf, obs_idx))
    if len(oo) != L + 1 or len(ok) != len(oi):
        raise PlpError(PLP_ERR_INVALID_ARG, "obs_offsets must have L + 1 entries, obs_kf and obs_idx one length")
    T = len(ok)
    ke, ko, le = array_or_none(kf_erased, np.uint8, F), array_or_none(kf_is_origin, np.uint8, F), array_or_none(lm_erased, np.uint8, L)
    cn = array_or_none(counts, np.int32, F)
    sg = np.ascontiguousarray(inv_level_sigma_sq, np.float32).reshape(-1)
    st = None if stop is None else np.ascontiguousarray(stop, np.int32).reshape(1)
    a = _struct(global_ba_args_c, dict(setup_type=int(setup_type), num_iter=int(num_iter), use_huber_kernel=int(bool(use_huber_kernel)), F=F, L=L, T=T, kp_stride=int(K),
                                       pose_stride=po.shape[1], num_levels=len(sg)), host_ptrs(
        inv_level_sigma_sq=sg, pose=po, kf_erased=ke, kf_is_origin=ko, undist=ku, x_right=xr, counts=cn, pos_w=pw, lm_erased=le, obs_offsets=oo, obs_kf=ok, obs_idx=oi,
        stop=st))
    a.camera = camera_model_c.from_buffer_copy(camera)
    return a, (po, ku, xr, pw, oo, ok, oi, ke, ko, le, cn, sg, st), F, L, T


def _global_ba_host(call, inputs, outputs, out):
    """the numpy side of plp_global_ba_host and plp_model_global_ba_host: call(args struct) runs the entry"""
    a, keep, F, L, T = _global_ba_inputs(**inputs)
    o = out_arrays(((k, shape(F, L, T), dt) for k, (shape, dt, optional) in GLOBAL_BA_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    set_outputs(a, GLOBAL_BA_OUTPUTS, o, host_ptr)
    call(a)
    return o


def _global_ba_kw(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin, lm_erased,
                  num_iter, use_huber_kernel, stop):
    return dict(camera=camera, setup_type=setup_type, pose=pose, undist=undist, pos_w=pos_w, obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx,
                inv_level_sigma_sq=inv_level_sigma_sq, x_right=x_right, counts=counts, kf_erased=kf_erased, kf_is_origin=kf_is_origin, lm_erased=lm_erased,
                num_iter=num_iter, use_huber_kernel=use_huber_kernel, stop=stop)


def _model_status_call(symbol):
    def call(a):
        r = getattr(lib(), symbol)(C.byref(a))
        if r != 1:
            raise PlpError(-r, lib().plp_last_error().decode())
    return call


def model_global_ba(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right=None, counts=None, kf_erased=None,
                    kf_is_origin=None, lm_erased=None, num_iter=10, use_huber_kernel=True, stop=None, outputs=None, out=None):
    """Host build of optimize::global_bundle_adjuster::optimize (csrc/global_ba.hpp; no GPU needed): the arguments and the result
    of matcher.global_ba."""
    return _global_ba_host(_model_status_call("plp_model_global_ba_host"), _global_ba_kw(
        camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right, counts, kf_erased, kf_is_origin, lm_erased, num_iter,
        use_huber_kernel, stop), outputs, out)


def _loop_ba_propagate_host(call, pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized, pos_after, kf_erased, kf_is_origin, lm_erased, out):
    po = np.ascontiguousarray(pose, np.float64)
    if po.ndim != 2 or po.shape[1] < 12:
        raise PlpError(PLP_ERR_INVALID_ARG, "pose must be (F, pose_stride >= 12)")
    F = po.shape[0]
    pw = np.ascontiguousarray(pos_w, np.float64).reshape(-1, 3)
    L = len(pw)
    kp, ko = np.ascontiguousarray(kf_parent, np.int32).reshape(F), np.ascontiguousarray(kf_optimized, np.uint8).reshape(F)
    pa = np.ascontiguousarray(pose_after, np.float64).reshape(F, 15)
    rk, lo = np.ascontiguousarray(ref_kf, np.int32).reshape(L), np.ascontiguousarray(lm_optimized, np.uint8).reshape(L)
    pq = np.ascontiguousarray(pos_after, np.float64).reshape(L, 3)
    ke, kg, le = array_or_none(kf_erased, np.uint8, F), array_or_none(kf_is_origin, np.uint8, F), array_or_none(lm_erased, np.uint8, L)
    o = out_arrays(((k, shape(F, L), dt) for k, (shape, dt) in LOOP_BA_PROPAGATE_OUTPUTS.items()), out)
    a = _struct(loop_ba_propagate_args_c, dict(F=F, L=L, pose_stride=po.shape[1]), host_ptrs(
        pose=po, kf_erased=ke, kf_is_origin=kg, kf_parent=kp, kf_optimized=ko, pose_after=pa, pos_w=pw, lm_erased=le, ref_kf=rk, lm_optimized=lo, pos_after=pq))
    set_outputs(a, LOOP_BA_PROPAGATE_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_loop_ba_propagate(pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized, pos_after, kf_erased=None, kf_is_origin=None, lm_erased=None,
                            out=None):
    """Host build of the loop adjuster's map update (module/loop_bundle_adjuster.cc:109-181; no GPU needed): the arguments and the result of
    matcher.loop_ba_propagate."""
    return _loop_ba_propagate_host(_model_status_call("plp_model_loop_ba_propagate_host"), pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized,
                                   pos_after, kf_erased, kf_is_origin, lm_erased, out)


def _chol_dense(call, A, b, lam):
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    n = len(b)
    if A.shape != (n, n):
        raise PlpError(PLP_ERR_INVALID_ARG, "A must be (n, n) and b (n,)")
    x = np.zeros(n)
    ok = np.zeros(1, np.int32)
    call(n, host_ptr(A), host_ptr(b), float(lam), host_ptr(x), host_ptr(ok))
    return x, bool(ok[0])


def model_chol_dense(A, b, lam=0.0):
    """Host build of D23's dense solve (A + lam I) x = b: the Cholesky in natural order and both substitutions (no GPU needed).  Returns (x, ok)."""
    def call(n, *rest):
        if lib().plp_model_chol_dense_host(n, *rest) != n:
            raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_chol_dense_host")
    return _chol_dense(call, A, b, lam)


class global_bundle_adjuster:
    """Mirror of optimize::global_bundle_adjuster (optimize/global_bundle_adjuster.h) over the point map: optimize() takes the map tables and returns the
    result dict of matcher.global_ba; mt: a matcher (the GPU entry), or None = the host build."""

    def __init__(self, num_iter=10, use_huber_kernel=True, mt=None):
        self.num_iter, self.use_huber_kernel, self._mt = int(num_iter), bool(use_huber_kernel), mt

    def optimize(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right=None, counts=None, kf_erased=None,
                 kf_is_origin=None, lm_erased=None, stop=None):
        fn = model_global_ba if self._mt is None else self._mt.global_ba
        return fn(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, x_right=x_right, counts=counts, kf_erased=kf_erased,
                  kf_is_origin=kf_is_origin, lm_erased=lm_erased, num_iter=self.num_iter, use_huber_kernel=self.use_huber_kernel, stop=stop)


class loop_bundle_adjuster:
    """Mirror of module::loop_bundle_adjuster (module/loop_bundle_adjuster.h), its array half: optimize() runs the global adjuster without the Huber kernel,
    carries the correction along the spanning tree and returns the tables a caller writes back."""

    def __init__(self, num_iter=10, mt=None):
        self.num_iter, self._mt = int(num_iter), mt

    def optimize(self, camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq, kf_parent, ref_kf, x_right=None, counts=None,
                 kf_erased=None, kf_is_origin=None, lm_erased=None, stop=None):
        """Returns dict(status, the global adjuster's result `ba`, and -- unless the status is GLOBAL_BA_STOPPED -- pose (F, 15), pose_before (F, 12), kf_status,
        pos_w (L, 3), lm_status: rows the update does not write hold the input's pose (with zeros behind its twelve entries) and position)."""
        ba = global_bundle_adjuster(self.num_iter, False, self._mt).optimize(camera, setup_type, pose, undist, pos_w, obs_offsets, obs_kf, obs_idx, inv_level_sigma_sq,
                                                                             x_right, counts, kf_erased, kf_is_origin, lm_erased, stop)
        r = dict(status=int(ba["status"][0]), ba=ba)
        if r["status"] == 2:                                 # GLOBAL_BA_STOPPED (:255-258): the map is not touched
            return r
        po = np.ascontiguousarray(pose, np.float64)
        out = dict(pose=np.zeros((len(po), 15)), pos_w=np.array(pos_w, np.float64).reshape(-1, 3))
        out["pose"][:, :12] = po[:, :12]
        fn = model_loop_ba_propagate if self._mt is None else self._mt.loop_ba_propagate
        r.update(fn(po, kf_parent, ba["kf_optimized"], ba["pose"], pos_w, ref_kf, ba["lm_optimized"], ba["pos_w"], kf_erased=kf_erased, kf_is_origin=kf_is_origin,
                    lm_erased=lm_erased, out=out))
        return r
