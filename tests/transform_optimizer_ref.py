"""Plain-Python restatement of DESIGN.md section 5, D16: optimize::transform_optimizer::optimize of the reference
(optimize/transform_optimizer.cc:47-197) with the edges of optimize/g2o/sim3/, g2o's Sim3 and g2o's Levenberg-Marquardt, written from those
sources and from D16.  What D15 fixes (the quaternion arithmetic, sin / cos, Huber, IEEE division and root) is tests/pose_optimizer_ref.py's.
Python floats only (IEEE f64, one rounding per operation, no fused multiply-add): the host build of csrc/transform_opt.hpp is held to this
bit for bit (tests/test_transform_optimizer_cpu.py)."""
import math

import pose_optimizer_ref as D15
from pose_optimizer_ref import DBL_MAX, END_ITERATIONS, END_RHO_ZERO, END_TRIES, MAX_TRIES, NAN, NUMERIC_DELTA, _div, f32

FIRST_ITERS = 5
MIN_INLIERS = 10
OK, TOO_FEW_INLIERS = 0, 1
EXP_DOMAIN = 700.0


# ---- exp
def exp(x):
    if not (-EXP_DOMAIN <= x <= EXP_DOMAIN):
        return NAN
    k = float(math.floor(x * 1.44269504088896338700e+00 + 0.5))
    hi = x - k * 6.93147180369123816490e-01
    lo = k * 1.90821492927058770002e-10
    r = hi - lo
    t = r * r
    c = r - t * (1.66666666666666019037e-01 + t * (-2.77777777770155933842e-03 + t * (6.61375632143793436117e-05 +
        t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    return y * math.ldexp(1.0, int(k))


# ---- the vertex; est = [qx, qy, qz, qw, tx, ty, tz, s]
def est_from_input(rot9, trans3, scale):
    return D15.quat_from_rot([float(v) for v in rot9]) + [float(v) for v in trans3] + [float(f32(scale))]


def sim3_map(est, p):
    r = D15.quat_rotate(est, p)
    return [est[7] * r[0] + est[4], est[7] * r[1] + est[5], est[7] * r[2] + est[6]]


def inverse(est):
    q = [-est[0], -est[1], -est[2], est[3]]
    c = _div(-1.0, est[7])
    return q + D15.quat_rotate(q, [c * est[4], c * est[5], c * est[6]]) + [_div(1.0, est[7])]


def mul(a, b):
    o = [0.0] * 8
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1]
    o[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2]
    o[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0]
    r = D15.quat_rotate(a, b[4:7])
    o[4], o[5], o[6] = a[7] * r[0] + a[4], a[7] * r[1] + a[5], a[7] * r[2] + a[6]
    o[7] = a[7] * b[7]
    return o


def sim3_branch(u, fix_scale=False):
    """which of the four branches of Sim3(update) the update takes: (|sigma| < eps, theta < eps)"""
    sigma = 0.0 if fix_scale else u[6]
    theta = D15._sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    return abs(sigma) < 0.00001, theta < 0.00001


def oplus(u, est, fix_scale=False):
    """Sim3(u) * est"""
    a, b, c = u[0], u[1], u[2]
    sigma = 0.0 if fix_scale else u[6]
    theta = D15._sqrt((a * a + b * b) + c * c)
    s = exp(sigma)
    O2 = [-(b * b + c * c), a * b, a * c, a * b, -(a * a + c * c), b * c, a * c, b * c, -(a * a + b * b)]
    O = [0.0, -c, b, c, 0.0, -a, -b, a, 0.0]
    eps = 0.00001
    k1 = k2 = 1.0
    si, co = 0.0, 1.0
    if not (theta < eps):
        si, co = D15.sincos(theta)
        k1 = _div(si, theta)
        k2 = _div(1.0 - co, theta * theta)
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 0.5, 1.0 / 6.0
        else:
            th2 = theta * theta
            A = _div(1.0 - co, th2)
            B = _div(theta - si, th2 * theta)
    else:
        C = _div(s - 1.0, sigma)
        sg2 = sigma * sigma
        if theta < eps:
            A = _div((sigma - 1.0) * s + 1.0, sg2)
            B = _div(((0.5 * sg2 - sigma) + 1.0) * s, sg2 * sigma)
        else:
            sa, sb = s * si, s * co
            th2 = theta * theta
            cc = th2 + sg2
            A = _div(sa * sigma + (1.0 - sb) * theta, theta * cc)
            B = _div(C - _div((sb - 1.0) * sigma + sa * theta, cc), th2)
    ident = [1.0 if i in (0, 4, 8) else 0.0 for i in range(9)]
    R = [(ident[i] + k1 * O[i]) + k2 * O2[i] for i in range(9)]
    W = [(A * O[i] + B * O2[i]) + C * ident[i] for i in range(9)]
    e = D15.quat_from_rot(R) + [(W[3 * i] * u[3] + W[3 * i + 1] * u[4]) + W[3 * i + 2] * u[5] for i in range(3)] + [s]
    return mul(e, est)


def linearisation_sims(est, fix_scale):
    """the fifteen similarities of a linearisation and their inverses"""
    sims = []
    for d in range(7):
        for v in (NUMERIC_DELTA, -NUMERIC_DELTA):
            u = [0.0] * 7
            u[d] = v
            sims.append(oplus(u, est, fix_scale))
    sims.append(list(est))
    return sims, [inverse(s) for s in sims]


# ---- the edges
class Cam:
    def __init__(self, fx, fy, cx, cy):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)


def to_camera(pose, pw):
    return [((pose[3 * i] * pw[0] + pose[3 * i + 1] * pw[1]) + pose[3 * i + 2] * pw[2]) + pose[9 + i] for i in range(3)]


def edge_error(sim, C, pc, ox, oy, w):
    """returns (chi2, (e0, e1))"""
    x, y, z = sim3_map(sim, pc)
    e0 = ox - (_div(C.fx * x, z) + C.cx)
    e1 = oy - (_div(C.fy * y, z) + C.cy)
    return e0 * (w * e0) + e1 * (w * e1), (e0, e1)


def terms(J, e, w, rho0, rho1):
    wr = rho1 * w
    o0, o1 = (-(w * e[0])) * rho1, (-(w * e[1])) * rho1
    T = []
    for i in range(7):
        for j in range(i, 7):
            T.append(J[i] * (wr * J[j]) + J[7 + i] * (wr * J[7 + j]))
    for i in range(7):
        T.append(J[i] * o0 + J[7 + i] * o1)
    T.append(rho0)
    return T


def edge_terms(sims, C, pc, ox, oy, w, delta):
    scalar = 1.0 / (2.0 * NUMERIC_DELTA)
    J = [0.0] * 14
    for d in range(7):
        _, p = edge_error(sims[2 * d], C, pc, ox, oy, w)
        _, m = edge_error(sims[2 * d + 1], C, pc, ox, oy, w)
        J[d] = scalar * (p[0] - m[0])
        J[7 + d] = scalar * (p[1] - m[1])
    chi2, e = edge_error(sims[14], C, pc, ox, oy, w)
    rho0, rho1 = D15.huber(chi2, delta)
    return chi2, terms(J, e, w, rho0, rho1)


# ---- the 7 x 7 solve
def h_index(i, j):
    return i * 7 - (i * (i - 1)) // 2 + (j - i)


def chol7(H28, b, lam):
    """(x, ok)"""
    n = 7
    Lf = [0.0] * (n * n)
    x = [0.0] * n
    y = [0.0] * n
    for j in range(n):
        s = H28[h_index(j, j)] + lam
        for k in range(j):
            s = s - Lf[n * j + k] * Lf[n * j + k]
        if not (s > 0.0) or s > DBL_MAX:
            return [0.0] * n, False
        d = math.sqrt(s)
        Lf[n * j + j] = d
        for i in range(j + 1, n):
            v = H28[h_index(j, i)]
            for k in range(j):
                v = v - Lf[n * i + k] * Lf[n * j + k]
            Lf[n * i + j] = v / d
    for i in range(n):
        v = b[i]
        for k in range(i):
            v = v - Lf[n * i + k] * y[k]
        y[i] = v / Lf[n * i + i]
    for i in range(n - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, n):
            v = v - Lf[n * k + i] * x[k]
        x[i] = v / Lf[n * i + i]
    return x, True


# ---- one problem
class Problem:
    """One pair in slot form.  slots: list of dict(valid, x1, y1, octave1, x2, y2, octave2 (key points idx1 and idx2; x, y already f32 values),
    pos_w_1, pos_w_2)."""

    def __init__(self, cam, fix_scale, pose_1, pose_2, rot_12, trans_12, scale_12, slots, inv_sigma_sq_1, inv_sigma_sq_2, chi_sq=10.0):
        self.cam, self.fix_scale = cam, bool(fix_scale)
        self.pose_1, self.pose_2 = [float(v) for v in pose_1], [float(v) for v in pose_2]
        self.rot_12, self.trans_12, self.scale_12 = [float(v) for v in rot_12], [float(v) for v in trans_12], float(f32(scale_12))
        self.slots = slots
        self.sig1 = [float(f32(v)) for v in inv_sigma_sq_1]
        self.sig2 = [float(f32(v)) for v in inv_sigma_sq_2]
        self.chi_sq = float(f32(chi_sq))
        self.delta = float(f32(math.sqrt(self.chi_sq)))        # std::sqrt(float): the f64 root rounded once more


def observations(Pb):
    return [s for s, m in enumerate(Pb.slots) if m["valid"] and 0 <= m["octave1"] < len(Pb.sig1) and 0 <= m["octave2"] < len(Pb.sig2)]


def _edges(Pb, s):
    """the two edges of slot s, forward then backward: (which similarities, pc, ox, oy, w)"""
    m = Pb.slots[s]
    return ((0, to_camera(Pb.pose_2, m["pos_w_2"]), m["x1"], m["y1"], Pb.sig1[m["octave1"]]),
            (1, to_camera(Pb.pose_1, m["pos_w_1"]), m["x2"], m["y2"], Pb.sig2[m["octave2"]]))


def _pass(Pb, obs, level, chi2, sims, invs, lin):
    """one pass over the kept matches in slot order, forward before backward: the 36 sums (lin) or the robust chi2 alone in sums[35]"""
    sums = [0.0] * 36
    for k, s in enumerate(obs):
        if level[k]:
            continue
        for d, pc, ox, oy, w in _edges(Pb, s):
            S = invs if d else sims
            if lin:
                chi2[2 * k + d], T = edge_terms(S, Pb.cam, pc, ox, oy, w, Pb.delta)
                for t in range(36):
                    sums[t] = sums[t] + T[t]
            else:
                chi2[2 * k + d] = edge_error(S[14], Pb.cam, pc, ox, oy, w)[0]
                sums[35] = sums[35] + D15.huber(chi2[2 * k + d], Pb.delta)[0]
    return sums


def linearize(Pb, active=None):
    """model_transform_linearize of one problem: (sums[36], {slot: (chi2_12, chi2_21)})"""
    obs = observations(Pb)
    level = [0 if active is None or active[s] else 1 for s in obs]
    chi2 = [NAN] * (2 * len(obs))
    sims, invs = linearisation_sims(est_from_input(Pb.rot_12, Pb.trans_12, Pb.scale_12), Pb.fix_scale)
    sums = _pass(Pb, obs, level, chi2, sims, invs, True)
    return sums, {s: (chi2[2 * k], chi2[2 * k + 1]) for k, s in enumerate(obs) if not level[k]}


def world_to_1(est, pose_2):
    m = mul(est, D15.quat_from_rot(pose_2) + [pose_2[9], pose_2[10], pose_2[11], 1.0])
    return D15.rot_from_quat(m) + m[4:8]


def optimize(Pb, num_iter=10, kept=None):
    """One problem.  kept: the caller's flag list (values of slots that are not written stay).  Returns dict(status, num_valid, num_inliers, rot_12,
    trans_12, scale_12, world_to_1, kept, round_info, round_chi2, census: what the run reached)."""
    flags = list(kept) if kept is not None else [0] * len(Pb.slots)
    info = [[0, 0, 0, 0], [0, 0, 0, 0]]
    rchi = [[0.0, 0.0], [0.0, 0.0]]
    census = dict(nan_outlier_round1=0, nan_inlier_round2=0, branches=set())
    obs = observations(Pb)
    n = len(obs)
    for s in obs:
        flags[s] = 1
    est0 = est_from_input(Pb.rot_12, Pb.trans_12, Pb.scale_12)
    res = dict(num_valid=n, kept=flags, round_info=info, round_chi2=rchi, census=census)

    def early():
        res.update(status=TOO_FEW_INLIERS, num_inliers=0, rot_12=list(Pb.rot_12), trans_12=list(Pb.trans_12), scale_12=Pb.scale_12,
                   world_to_1=world_to_1(est0, Pb.pose_2))
        return res
    if n == 0:
        return early()
    est = est0
    level = [0] * n
    chi2 = [0.0] * (2 * n)
    left = n
    lam, ni, current_chi = 0.0, 2.0, 0.0
    for rnd in range(2):
        iterations = rejected = end = 0
        for it in range(FIRST_ITERS if rnd == 0 else num_iter):
            sims, invs = linearisation_sims(est, Pb.fix_scale)
            S = _pass(Pb, obs, level, chi2, sims, invs, True)
            current_chi = S[35]
            if it == 0:
                m = 0.0
                for j in range(7):
                    d = abs(S[h_index(j, j)])
                    m = d if d > m else m
                lam = 1e-5 * m
                ni = 2.0
            qmax = 0
            rho = 0.0
            while True:
                bak = est
                x, ok2 = chol7(S[:28], S[28:35], lam)
                census["branches"].add(sim3_branch(x, Pb.fix_scale))
                est = oplus(x, bak, Pb.fix_scale)
                tried = [None] * 14 + [est]
                temp_sum = _pass(Pb, obs, level, chi2, tried, [None] * 14 + [inverse(est)], False)[35]
                temp_chi = temp_sum if ok2 else DBL_MAX
                scale = 0.0
                for j in range(7):
                    scale = scale + x[j] * (lam * x[j] + S[28 + j])
                scale = scale + 1e-3
                rho = _div(current_chi - temp_chi, scale)
                if rho > 0.0 and -DBL_MAX <= temp_chi <= DBL_MAX:
                    v = 2.0 * rho - 1.0
                    alpha = 1.0 - (v * v) * v
                    alpha = alpha if alpha < 2.0 / 3.0 else 2.0 / 3.0
                    lam = lam * (alpha if alpha > 1.0 / 3.0 else 1.0 / 3.0)
                    ni = 2.0
                    current_chi = temp_chi
                else:
                    lam = lam * ni
                    ni = ni * 2.0
                    est = bak
                    rejected += 1
                qmax += 1
                if not (rho < 0.0 and qmax < MAX_TRIES):
                    break
            iterations += 1
            end = END_TRIES if qmax == MAX_TRIES else END_RHO_ZERO if rho == 0.0 else 0
            if end:
                break
        drops = 0
        for k, s in enumerate(obs):
            if level[k]:
                continue
            c12, c21 = chi2[2 * k], chi2[2 * k + 1]
            nan = c12 != c12 or c21 != c21
            if rnd == 0:
                drop = not (c12 < Pb.chi_sq and c21 < Pb.chi_sq)
                census["nan_outlier_round1"] += int(nan)
            else:
                drop = Pb.chi_sq < c12 or Pb.chi_sq < c21
                census["nan_inlier_round2"] += int(nan and not drop)
            if drop:
                level[k] = 1
                flags[s] = 0
                drops += 1
        left -= drops
        info[rnd] = [iterations, rejected, drops, end if end else END_ITERATIONS]
        rchi[rnd] = [current_chi, lam]
        if rnd == 0 and left < MIN_INLIERS:
            return early()
    res.update(status=OK, num_inliers=left, rot_12=D15.rot_from_quat(est), trans_12=est[4:7], scale_12=est[7], world_to_1=world_to_1(est, Pb.pose_2))
    return res
