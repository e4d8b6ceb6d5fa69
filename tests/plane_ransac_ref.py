"""Restatement of DESIGN.md section 5, D19 in plain Python / numpy, written from the definition and the reference's text, not from
csrc/plane_fit.hpp: estimate_plane_SVD (planar_mapping_module.cc:735-771) as D19 item 3 writes it down, the draws of item 2, the sums of
item 4, the literal serial loops of estimate_plane_sequential_RANSAC (:412-591, behind create_new_plane's gate :359) and
update_plane_via_RANSAC (:593-733), and refine_points (:954-1004).  numpy is used for elementwise IEEE operations only (+ - * / sqrt on
float64 arrays, one ufunc per operation: nothing is fused and no numpy reduction is called); every sum is chained here."""
import math

import numpy as np

from pnp_solver_ref import sym_jacobi              # D14's one-sided Jacobi, which D19 item 3 uses at n = 3

CREATE, UPDATE = 0, 1
OK, TOO_FEW_POINTS, NO_ELIGIBLE, NOT_FOUND, ERROR_ABOVE_THRESHOLD, TOO_FEW_LEFT = range(6)
LM_ERASED, LM_OWNED = 1, 2
FLAG_INVALID, FLAG_NEED_REFINEMENT, FLAG_GATED = 1, 2, 4
DBL_MAX = float(np.finfo(np.float64).max)
MASK = (1 << 64) - 1
SENTINEL = dict(status=0xEE, flags=0xEE, equation=-7.25, best_error=-7.25, best_iter=-77, last_iter=-77, num_inliers=-77, inliers=0xEE,
                hyp_residual=-7.25, hyp_inliers=-77, hyp_error=-7.25)
DTYPES = dict(status=np.uint8, flags=np.uint8, equation=np.float64, best_error=np.float64, best_iter=np.int32, last_iter=np.int32,
              num_inliers=np.int32, inliers=np.uint8, hyp_residual=np.float64, hyp_inliers=np.int32, hyp_error=np.float64)


# ---- item 2: the draws
def mix64(x):
    x &= MASK
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def draw(seed, p, it, k, n_eligible):
    """rank k of hypothesis `it` of problem p"""
    base = mix64((seed & MASK) ^ mix64(((p & 0xFFFFFFFF) << 32) | (it & 0xFFFFFFFF)))
    r = mix64(base + (k + 1) * 0x9E3779B97F4A7C15)
    return (r >> 32) % n_eligible


def sample_size(mode, n, points_per_ransac):
    if mode == CREATE:
        return points_per_ransac
    m = 0
    while float(m) < float(n) * 0.8:               # `while (indexes.size() < lms.size() * 0.8)` (:620)
        m += 1
    return m


# ---- item 4: a sum over a list
def sum64(v):
    """64 partial chains (k = j mod 64, ascending, from 0.0), then one chain over j = 0 .. 63"""
    part = np.zeros(64)
    for r in range(0, len(v), 64):
        seg = v[r:r + 64]
        part[:len(seg)] = part[:len(seg)] + seg
    t = 0.0
    for j in range(64):
        t = t + float(part[j])
    return t


# ---- item 3: the fit
def normal_of(C):
    """C: the six scatter entries (00, 01, 02, 11, 12, 22).  Returns (unit normal with its sign fixed, sweeps)"""
    A = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    _, Ut, sweeps = sym_jacobi(A)
    v = list(Ut[2])
    n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    if n2 > 0.0:
        nn = math.sqrt(n2)
        v = [v[0] / nn, v[1] / nn, v[2] / nn]
    big, mag = v[0], abs(v[0])
    for i in (1, 2):
        if abs(v[i]) > mag:
            big, mag = v[i], abs(v[i])
    if big < 0.0:
        v = [-v[0], -v[1], -v[2]]
    return v, sweeps


def fit(X):
    """X: (m, 3) points in list order, m >= 1.  Returns (equation [a, b, c, d], residual, sweeps)"""
    with np.errstate(all="ignore"):
        X = np.asarray(X, np.float64)
        m = float(len(X))
        c = [sum64(X[:, r]) / m for r in range(3)]
        xc = [X[:, r] - c[r] for r in range(3)]
        C = [sum64(xc[0] * xc[0]), sum64(xc[0] * xc[1]), sum64(xc[0] * xc[2]), sum64(xc[1] * xc[1]), sum64(xc[1] * xc[2]), sum64(xc[2] * xc[2])]
        nrm, sweeps = normal_of(C)
        d = -((nrm[0] * c[0] + nrm[1] * c[1]) + nrm[2] * c[2])
        e = ((nrm[0] * X[:, 0] + nrm[1] * X[:, 1]) + nrm[2] * X[:, 2]) + d
        s = sum64(e * e)
        residual = abs(math.sqrt(s) / m) if s == s and s >= 0.0 else float("nan")
    return [nrm[0], nrm[1], nrm[2], d], residual, sweeps


def distance(eq, X):
    """Plane::calculate_distance (landmark_plane.cc:118-123) with set_equation's _abs_n (:106), for the rows of X"""
    with np.errstate(all="ignore"):
        abs_n = np.sqrt(np.float64((eq[0] * eq[0] + eq[1] * eq[1]) + eq[2] * eq[2]))
        X = np.asarray(X, np.float64).reshape(-1, 3)
        return np.abs((((eq[0] * X[:, 0] + eq[1] * X[:, 1]) + eq[2] * X[:, 2]) + eq[3]) / abs_n)


# ---- the two loops
def ransac(mode, pos_w, flags, dist_thresh, error_thresh, points_per_ransac=18, min_points_before_ransac=12, iters=50, inliers_ratio_thr=0.7,
           best_error_in=None, equation_in=None, samples=None, seed=0, p=0, record=None):
    """One plane.  pos_w (n, 3), flags (n,): the entries of lms in slot order.  samples: (iters, >= m) ranks or None.  Returns dict of the
    outputs that are defined (a key absent = the library leaves the caller's value), `hyp_*` for every iteration, and `trace`.  record: a list that
    receives the point list of every fit."""
    pos_w = np.asarray(pos_w, np.float64).reshape(-1, 3)
    flags = np.asarray(flags, np.uint8).reshape(-1)
    n = len(flags)
    erased = (flags & LM_ERASED) != 0
    owned = (flags & LM_OWNED) != 0
    eligible = np.flatnonzero(~erased if mode == CREATE else (~erased & owned))
    o = dict(best_iter=-1, last_iter=-1, num_inliers=0, inliers=np.zeros(n, np.uint8), hyp_residual=np.zeros(iters), hyp_inliers=np.zeros(iters, np.int32),
             hyp_error=np.full(iters, DBL_MAX), flags=0, trace=dict(gate=False, broke_at=None, accepted=[], ran=0))
    if mode == UPDATE:
        o["equation"], o["best_error"] = [float(x) for x in equation_in], float(best_error_in)
    # before the loop
    if mode == CREATE and n < min_points_before_ransac:        # create_new_plane (:359)
        o["status"], o["flags"] = TOO_FEW_POINTS, FLAG_GATED
        o["trace"]["gate"] = True
        return o
    if n == 0:                                                 # :423, :597
        o["status"] = TOO_FEW_POINTS
        return o
    if n < points_per_ransac:                                  # :428, :602
        o["status"], o["flags"] = TOO_FEW_POINTS, (FLAG_INVALID if mode == UPDATE else 0)
        return o
    if len(eligible) == 0:                                     # the reference's while loop would not end (D19 item 2)
        o["status"] = NO_ELIGIBLE
        return o
    m = sample_size(mode, n, points_per_ransac)
    cache = {}

    def sample_fit(i):
        ranks = [int(samples[i][k]) if samples is not None else draw(seed, p, i, k, len(eligible)) for k in range(m)]
        if any(r < 0 or r >= len(eligible) for r in ranks):
            return [0.0, 0.0, 0.0, 0.0], DBL_MAX
        if record is not None:
            record.append(pos_w[eligible[ranks]].copy())
        eq, res, _ = fit(pos_w[eligible[ranks]])
        return eq, res

    def hypothesis(i):
        """what iteration i computes from the inputs alone: (sample equation, residual, inliers_list, gate, refit equation, error)"""
        if i not in cache:
            eq, res = sample_fit(i)
            dist = distance(eq, pos_w)
            inliers_list = [j for j in range(n) if not erased[j] and dist[j] < dist_thresh]       # [2]
            if mode == CREATE:
                inlier_ratio = float(len(inliers_list)) / float(n)
                gate = inlier_ratio > inliers_ratio_thr and len(inliers_list) >= points_per_ransac
            else:
                gate = len(inliers_list) >= points_per_ransac
            eq_r, err = [0.0] * 4, DBL_MAX
            if gate:
                if record is not None:
                    record.append(pos_w[inliers_list].copy())
                eq_r, err, _ = fit(pos_w[inliers_list])
            cache[i] = (eq, res, inliers_list, gate, eq_r, err)
        return cache[i]

    best_error = DBL_MAX if mode == CREATE else float(best_error_in)
    best_inliers_list, best_found = [], False
    plane_eq, plane_best_error = None, None
    for i in range(iters):
        eq, residual, inliers_list, gate, eq_r, error = hypothesis(i)
        o["trace"]["ran"] = i + 1
        o["last_iter"] = i
        if residual < best_error:                              # :465, :641
            best_error = residual
        plane_eq, plane_best_error = eq, residual              # set_equation, set_best_error(residual) (:473-474, :649-650)
        if gate:                                               # [3]
            if error < best_error:
                best_error = error
                plane_eq, plane_best_error = eq_r, best_error
                best_inliers_list = list(inliers_list)
                best_found = True
                o["best_iter"] = i
                o["trace"]["accepted"].append(i)
                if mode == CREATE and error < error_thresh:    # :526
                    o["trace"]["broke_at"] = i
                    break
    for i in range(iters):                                     # the records of every hypothesis, reached or not
        _, res, lst, gate, _, err = hypothesis(i)
        o["hyp_residual"][i], o["hyp_inliers"][i], o["hyp_error"][i] = res, len(lst), err
    o["equation"], o["best_error"] = plane_eq, plane_best_error
    if not best_found:                                         # :545, :698
        o["status"], o["flags"] = NOT_FOUND, (FLAG_NEED_REFINEMENT if mode == UPDATE else 0)
        return o
    if best_error > error_thresh:                              # :554, :698
        o["status"], o["flags"] = ERROR_ABOVE_THRESHOLD, (FLAG_NEED_REFINEMENT if mode == UPDATE else 0)
        return o
    dist = distance(plane_eq, pos_w)                           # [4]
    kept = [j for j in best_inliers_list if not erased[j] and dist[j] < dist_thresh]
    o["inliers"][kept] = 1
    o["num_inliers"] = len(kept)
    if mode == UPDATE and len(kept) < points_per_ransac:       # :722
        o["status"], o["flags"] = TOO_FEW_LEFT, FLAG_INVALID
        return o
    o["status"] = OK
    return o


def expected(results, n_cap, iters):
    """the arrays of a call over these problems' results, from sentinel-filled outputs"""
    P = len(results)
    shape = dict(equation=(P, 4), inliers=(P, n_cap), hyp_residual=(P, iters), hyp_inliers=(P, iters), hyp_error=(P, iters))
    out = {k: np.full(shape.get(k, (P,)), SENTINEL[k], DTYPES[k]) for k in SENTINEL}
    for p, r in enumerate(results):
        for k in SENTINEL:
            if k not in r:
                continue
            if k == "inliers":
                out[k][p, :len(r[k])] = r[k]
            else:
                out[k][p] = r[k]
    return out


def refine_points(pos_w, lm_plane, flags, equation, active, dist_thresh):
    """refine_points (:954-1004) over a landmark list.  Returns (new pos_w, changed)"""
    pos = np.array(pos_w, np.float64).reshape(-1, 3)
    changed = np.zeros(len(pos), np.uint8)
    equation = np.asarray(equation, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        for i in range(len(pos)):
            pl = int(lm_plane[i])
            if pl < 0 or pl >= len(equation) or not active[pl]:
                continue
            if (flags[i] & LM_ERASED) or not (flags[i] & LM_OWNED):                   # :970
                continue
            eq = [float(x) for x in equation[pl]]
            x = [float(v) for v in pos[i]]
            n2 = (eq[0] * eq[0] + eq[1] * eq[1]) + eq[2] * eq[2]
            abs_n = math.sqrt(n2) if n2 >= 0.0 else float("nan")
            fdiv = lambda a, b: float(np.float64(a) / np.float64(b))
            dist_of = lambda q: abs(fdiv(((eq[0] * q[0] + eq[1] * q[1]) + eq[2] * q[2]) + eq[3], abs_n))
            dist_old = dist_of(x)                                                     # :976
            if not (abs(dist_old) > 0.0):                                             # :977
                continue
            nn = [fdiv(eq[r], abs_n) for r in range(3)] if n2 > 0.0 else eq[:3]       # get_normal().normalized() (:982)
            y = [x[r] - nn[r] * dist_old for r in range(3)]                           # :983
            dist_new = dist_of(y)                                                     # :984
            if dist_new < dist_thresh and dist_new < dist_old:                        # :985-986
                pos[i] = y
                changed[i] = 1
    return pos, changed
