"""Map initialisation and the robust match: solve::essential_solver (include/plp_front.h: plp_essential_ransac_*, the plp_model_essential_* host
builds): the numpy side of the host-pointer entry and the host builds, and the mirror class under the reference's name."""

import numpy as np

from ._abi import ESSENTIAL_OK, _struct, essential_ransac_args_c
from ._core import PLP_ERR_INVALID_ARG, PlpError, lib
from ._marshal import array_or_none, host_ptr, host_ptrs, model_call, model_draw, out_arrays, set_outputs, wanted

# the outputs of plp_essential_ransac_*: name -> (shape per problem given (n_cap, iters), dtype, optional)
ESSENTIAL_OUTPUTS = dict(status=(lambda M, I: (), np.uint8, False), num_matches=(lambda M, I: (), np.int32, False), E_21=(lambda M, I: (3, 3), np.float64, False),
                         score=(lambda M, I: (), np.float32, False), num_inliers=(lambda M, I: (), np.int32, False), best_iter=(lambda M, I: (), np.int32, False),
                         inliers=(lambda M, I: (M,), np.uint8, True), hyp_score=(lambda M, I: (I,), np.float32, True))


def _essential_ransac_host(call, bearing_1, bearing_2, match, iters, recompute, samples, seed, counts_1, counts_2, outputs, out):
    """the numpy side of plp_essential_ransac_host and plp_model_essential_ransac_host: call(args struct) runs the entry"""
    ma = np.ascontiguousarray(match, np.int32)
    if ma.ndim != 2:
        raise PlpError(PLP_ERR_INVALID_ARG, "match must be (P, n_cap)")
    P_, M = ma.shape
    b1 = np.ascontiguousarray(bearing_1, np.float64).reshape(P_, M, 3)
    b2 = np.ascontiguousarray(bearing_2, np.float64)
    b2 = b2.reshape(P_, -1, 3) if P_ else b2.reshape(0, 0, 3)
    I = int(iters)
    sm = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(P_, I, 8)
    c1, c2 = array_or_none(counts_1, np.int32, P_), array_or_none(counts_2, np.int32, P_)
    o = out_arrays(((k, (P_,) + shape(M, max(I, 0)), dt) for k, (shape, dt, optional) in ESSENTIAL_OUTPUTS.items() if wanted(k, optional, outputs)), out)
    a = _struct(essential_ransac_args_c, dict(P=P_, n_cap=M, m_cap=b2.shape[1], iters=I, recompute=int(bool(recompute)), seed=int(seed) & 0xFFFFFFFFFFFFFFFF),
                host_ptrs(counts_1=c1, counts_2=c2, bearing_1=b1, bearing_2=b2, match=ma, samples=sm))
    set_outputs(a, ESSENTIAL_OUTPUTS, o, host_ptr)
    call(a)
    return o


def model_essential_ransac(bearing_1, bearing_2, match, iters=100, recompute=True, samples=None, seed=0, counts_1=None, counts_2=None, outputs=None, out=None):
    """Host build of solve::essential_solver's find_via_ransac (csrc/essential.hpp; no GPU needed): the arguments and
    the result of matcher.essential_ransac."""
    return _essential_ransac_host(model_call("plp_model_essential_ransac_host", "P"), bearing_1, bearing_2, match, iters, recompute, samples, seed, counts_1,
                                  counts_2, outputs, out)


def model_essential_fit(bearing_1, bearing_2, offsets=None):
    """Host build of essential_solver::compute_E_21 (solve/essential_solver.cc:121-154; D24 items b and c; no GPU needed) for lists of bearing
    pairs: bearing_1 / bearing_2 (n_rows, 3); list i holds rows offsets[i] .. offsets[i+1] (offsets None: one list of all rows).  Returns
    dict(E_21 (n, 3, 3), sweeps (n, 2): the 9 x 9 and the 3 x 3 Jacobi), without the leading axis for offsets None."""
    b1 = np.ascontiguousarray(bearing_1, np.float64).reshape(-1, 3); b2 = np.ascontiguousarray(bearing_2, np.float64).reshape(-1, 3)
    if len(b1) != len(b2):
        raise PlpError(PLP_ERR_INVALID_ARG, "bearing_1 and bearing_2 must hold the same number of rows")
    single = offsets is None
    off = np.array([0, len(b1)], np.int32) if single else np.ascontiguousarray(offsets, np.int32).reshape(-1)
    n = len(off) - 1
    if n < 0 or (n and int(off[-1]) > len(b1)):
        raise PlpError(PLP_ERR_INVALID_ARG, "offsets must be ascending within the rows")
    o = dict(E_21=np.zeros((n, 3, 3)), sweeps=np.zeros((n, 2), np.int32))
    if lib().plp_model_essential_fit_host(host_ptr(b1), host_ptr(b2), host_ptr(off), n, host_ptr(o["E_21"]), host_ptr(o["sweeps"])) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "offsets must be ascending within the rows")
    return {k: v[0] for k, v in o.items()} if single else o


def model_essential_check(bearing_1, bearing_2, match, E_21):
    """Host build of essential_solver::check_inliers (solve/essential_solver.cc:196-253; no GPU needed) of n matrices against one problem:
    bearing_1 (n_cap, 3), bearing_2 (m_cap, 3), match (n_cap,), E_21 (n, 3, 3) or (3, 3).  Returns dict(score (n,) f32, num_inliers (n,),
    inliers (n, n_cap) u8 in slot order), without the leading axis for one matrix."""
    ma = np.ascontiguousarray(match, np.int32).reshape(-1)
    b1 = np.ascontiguousarray(bearing_1, np.float64).reshape(len(ma), 3); b2 = np.ascontiguousarray(bearing_2, np.float64).reshape(-1, 3)
    E = np.ascontiguousarray(E_21, np.float64)
    single = E.ndim == 2
    E = E.reshape(-1, 3, 3)
    n = len(E)
    o = dict(score=np.zeros(n, np.float32), num_inliers=np.zeros(n, np.int32), inliers=np.zeros((n, len(ma)), np.uint8))
    if lib().plp_model_essential_check_host(host_ptr(b1), host_ptr(b2), host_ptr(ma), len(ma), len(b2), host_ptr(E), n, host_ptr(o["score"]),
                                            host_ptr(o["num_inliers"]), host_ptr(o["inliers"])) != n:
        raise PlpError(PLP_ERR_INVALID_ARG, "plp_model_essential_check_host")
    return {k: v[0] for k, v in o.items()} if single else o


def model_essential_draw(seed, p, iters, num_matches, iter0=0):
    """The samples plp_essential_ransac_* draw for problem p when the caller passes none (D24's generator; no GPU needed): (iters, 8) i32"""
    return model_draw("plp_model_essential_draw_host", "num_matches must be at least 8, iters non-negative", seed, p, iters, iter0, 8, num_matches)


class essential_solver:
    """Mirror of solve::essential_solver (solve/essential_solver.h): bearings_1 (n1, 3), bearings_2 (n2, 3), matches_12 a list of (idx1, idx2)
    pairs in ascending idx1 (as both callers of the reference build it), every idx1 at most once.  mt: a matcher (the GPU entry), or None = the
    host build.  samples / seed: as matcher.essential_ransac."""

    def __init__(self, bearings_1, bearings_2, matches_12, mt=None, samples=None, seed=0):
        b1 = np.ascontiguousarray(bearings_1, np.float64).reshape(-1, 3)
        b2 = np.ascontiguousarray(bearings_2, np.float64).reshape(-1, 3)
        m = np.asarray(matches_12, np.int64).reshape(-1, 2)
        if len(m) and (np.any(np.diff(m[:, 0]) <= 0) or m[:, 0].min() < 0 or m[:, 0].max() >= len(b1) or m[:, 1].min() < 0 or m[:, 1].max() >= len(b2)):
            raise PlpError(PLP_ERR_INVALID_ARG, "matches_12 must name key points of both frames, in strictly ascending idx1")
        match = np.full((1, max(len(b1), 1)), -1, np.int32)
        match[0, m[:, 0]] = m[:, 1]
        self._idx1 = m[:, 0].copy()
        self._in = (b1.reshape(1, -1, 3) if len(b1) else np.zeros((1, 1, 3)), b2.reshape(1, -1, 3) if len(b2) else np.zeros((1, 1, 3)), match)
        self._kw = dict(samples=samples, seed=seed)
        self._mt = mt
        self._r = None

    def find_via_ransac(self, max_num_iter, recompute=True):
        fn = model_essential_ransac if self._mt is None else self._mt.essential_ransac
        self._r = fn(*self._in, iters=int(max_num_iter), recompute=recompute, **self._kw)

    def solution_is_valid(self):
        return self._r is not None and int(self._r["status"][0]) == ESSENTIAL_OK

    def get_best_E_21(self):
        return self._r["E_21"][0].copy()

    def get_best_score(self):
        return float(self._r["score"][0])

    def get_inlier_matches(self):
        """is_inlier_match_: one flag per match of matches_12, in its order"""
        return self._r["inliers"][0, self._idx1].astype(bool)
