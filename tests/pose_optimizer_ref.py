"""Plain-Python restatement of DESIGN.md section 5, D15: optimize::pose_optimizer::optimize and pose_optimizer_extended_line::optimize of the
reference (optimize/pose_optimizer.cc:53-229, pose_optimizer_extended_line.cc:62-305) with the edges of optimize/g2o/se3/ and g2o's
Levenberg-Marquardt, written from those sources and from D15.  Python floats only (IEEE f64, one rounding per operation, no fused
multiply-add): the host build of csrc/pose_opt.hpp is held to this bit for bit (tests/test_pose_optimizer_cpu.py)."""
import math
import struct

NAN = float("nan")
DBL_MAX = 1.7976931348623157e308


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


CHI_SQ_2D = f32(5.99146)
CHI_SQ_3D = f32(7.81473)
DELTA_2D = f32(math.sqrt(CHI_SQ_2D))      # std::sqrt(float): correctly rounded, and so is the f64 root rounded once more
DELTA_3D = f32(math.sqrt(CHI_SQ_3D))
NUMERIC_DELTA = 1e-9
MAX_TRIES = 10
MIN_OBS = 5
END_ITERATIONS, END_TRIES, END_RHO_ZERO = 1, 2, 3


# ---- item 1: sin and cos
def sincos(x):
    if not (-1048576.0 <= x <= 1048576.0):
        return NAN, NAN
    k = float(math.floor(x * 6.36619772367581382433e-01 + 0.5))
    r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11
    z = r * r
    ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 +
         z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))))
    pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 +
         z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))))
    sr = r + (r * z) * ps
    cr = 1.0 - (0.5 * z - (z * z) * pc)
    q = int(k) & 3
    return (sr, cr, -sr, -cr)[q], (cr, -sr, -cr, sr)[q]


# ---- item 1: the vertex; est = [qx, qy, qz, qw, tx, ty, tz]
def quat_from_rot(R):
    t = (R[0] + R[4]) + R[8]
    q = [0.0] * 4
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[7] - R[5]) * t
        q[1] = (R[2] - R[6]) * t
        q[2] = (R[3] - R[1]) * t
        return q
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = _sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0)
    q[i] = 0.5 * t
    t = _div(0.5, t)
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def _sqrt(v):
    """IEEE sqrt: NaN for a negative or NaN argument"""
    if v != v or v < 0.0:
        return NAN
    return math.sqrt(v)


def _div(a, b):
    """IEEE division"""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def quat_normalize(q):
    if q[3] < 0.0:
        q = [-q[0], -q[1], -q[2], -q[3]]
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    if n2 > 0.0:
        n = math.sqrt(n2)
        q = [q[0] / n, q[1] / n, q[2] / n, q[3] / n]
    return list(q)


def rot_from_quat(q):
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def quat_rotate(q, v):
    ux = q[1] * v[2] - q[2] * v[1]
    uy = q[2] * v[0] - q[0] * v[2]
    uz = q[0] * v[1] - q[1] * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return [(v[0] + q[3] * ux) + (q[1] * uz - q[2] * uy),
            (v[1] + q[3] * uy) + (q[2] * ux - q[0] * uz),
            (v[2] + q[3] * uz) + (q[0] * uy - q[1] * ux)]


def se3_map(est, p):
    r = quat_rotate(est, p)
    return [r[0] + est[4], r[1] + est[5], r[2] + est[6]]


def est_from_pose(pose12):
    return quat_normalize(quat_from_rot(pose12)) + [pose12[9], pose12[10], pose12[11]]


def pose_from_est(est):
    R = rot_from_quat(est)
    t = [est[4], est[5], est[6]]
    cc = [((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2] for i in range(3)]
    return R + t + cc


def oplus(u, est):
    """SE3Quat::exp(u) * est"""
    a, b, c = u[0], u[1], u[2]
    theta = _sqrt((a * a + b * b) + c * c)
    O2 = [-(b * b + c * c), a * b, a * c, a * b, -(a * a + c * c), b * c, a * c, b * c, -(a * a + b * b)]
    O = [0.0, -c, b, c, 0.0, -a, -b, a, 0.0]
    if theta < 0.00001:
        k1, k2, v1, v2 = 1.0, 0.5, 0.5, 1.0 / 6.0
    else:
        s, co = sincos(theta)
        th2 = theta * theta
        k1 = s / theta
        k2 = (1.0 - co) / th2
        v1 = k2
        v2 = (theta - s) / (th2 * theta)
    R = [((1.0 if i in (0, 4, 8) else 0.0) + k1 * O[i]) + k2 * O2[i] for i in range(9)]
    V = [((1.0 if i in (0, 4, 8) else 0.0) + v1 * O[i]) + v2 * O2[i] for i in range(9)]
    e = quat_normalize(quat_from_rot(R))
    et = [(V[3 * i] * u[3] + V[3 * i + 1] * u[4]) + V[3 * i + 2] * u[5] for i in range(3)]
    p = est
    o = [0.0] * 7
    o[3] = ((e[3] * p[3] - e[0] * p[0]) - e[1] * p[1]) - e[2] * p[2]
    o[0] = ((e[3] * p[0] + e[0] * p[3]) + e[1] * p[2]) - e[2] * p[1]
    o[1] = ((e[3] * p[1] + e[1] * p[3]) + e[2] * p[0]) - e[0] * p[2]
    o[2] = ((e[3] * p[2] + e[2] * p[3]) + e[0] * p[1]) - e[1] * p[0]
    r = quat_rotate(e, p[4:7])
    return quat_normalize(o[:4]) + [et[0] + r[0], et[1] + r[1], et[2] + r[2]]


# ---- item 2: the edges
class Cam:
    def __init__(self, fx, fy, cx, cy, fxb):
        self.fx, self.fy, self.cx, self.cy, self.fxb = float(fx), float(fy), float(cx), float(cy), float(fxb)
        self.k20, self.k21, self.k22 = (-self.fy) * self.cx, (-self.fx) * self.cy, self.fx * self.fy


def point_error(est, C, pos_w, ox, oy, orr, mono, w):
    """returns (chi2, pos_c, e)"""
    x, y, z = se3_map(est, pos_w)
    rx = _div(C.fx * x, z) + C.cx
    e0 = ox - rx
    e1 = oy - (_div(C.fy * y, z) + C.cy)
    if mono:
        return e0 * (w * e0) + e1 * (w * e1), (x, y, z), (e0, e1, 0.0)
    e2 = orr - (rx - _div(C.fxb, z))
    return (e0 * (w * e0) + e1 * (w * e1)) + e2 * (w * e2), (x, y, z), (e0, e1, e2)


def huber(e2, delta):
    dsqr = delta * delta
    if e2 <= dsqr:
        return e2, 1.0
    sqrte = _sqrt(e2)
    return (2.0 * sqrte) * delta - dsqr, _div(delta, sqrte)


def terms(J, rows, e, w, rho0, rho1):
    wr = rho1 * w
    o = [(-(w * e[k])) * rho1 for k in range(3)]
    T = []
    for i in range(6):
        for j in range(i, 6):
            v = J[i] * (wr * J[j]) + J[6 + i] * (wr * J[6 + j])
            if rows == 3:
                v = v + J[12 + i] * (wr * J[12 + j])
            T.append(v)
    for i in range(6):
        v = J[i] * o[0] + J[6 + i] * o[1]
        if rows == 3:
            v = v + J[12 + i] * o[2]
        T.append(v)
    T.append(rho0)
    return T


def point_jacobian(C, pc):
    x, y, z = pc
    z_sq = z * z
    J = [0.0] * 18
    J[0] = _div(x * y, z_sq) * C.fx
    J[1] = (-(1.0 + _div(x * x, z_sq))) * C.fx
    J[2] = _div(y, z) * C.fx
    J[3] = _div(-1.0, z) * C.fx
    J[5] = _div(x, z_sq) * C.fx
    J[6] = (1.0 + _div(y * y, z_sq)) * C.fy
    J[7] = _div((-x) * y, z_sq) * C.fy
    J[8] = _div(-x, z) * C.fy
    J[10] = _div(-1.0, z) * C.fy
    J[11] = _div(y, z_sq) * C.fy
    J[12] = J[0] - _div(C.fxb * y, z_sq)
    J[13] = J[1] + _div(C.fxb * x, z_sq)
    J[14] = J[2]
    J[15] = J[3]
    J[17] = J[5] - _div(C.fxb, z_sq)
    return J


def point_terms(est, C, pos_w, ox, oy, orr, mono, w, robust, delta):
    chi2, pc, e = point_error(est, C, pos_w, ox, oy, orr, mono, w)
    rho0, rho1 = huber(chi2, delta) if robust else (chi2, 1.0)
    return chi2, terms(point_jacobian(C, pc), 2 if mono else 3, e, w, rho0, rho1)


def line_error(est, C, L, xs, ys, xe, ye, w):
    """returns (chi2, (e0, e1))"""
    R = rot_from_quat(est)
    tx, ty, tz = est[4], est[5], est[6]
    M = [[(-tz) * R[3 + j] + ty * R[6 + j] for j in range(3)],
         [tz * R[j] + (-tx) * R[6 + j] for j in range(3)],
         [(-ty) * R[j] + tx * R[3 + j] for j in range(3)]]
    top = [((((R[3 * i] * L[0] + R[3 * i + 1] * L[1]) + R[3 * i + 2] * L[2]) + M[i][0] * L[3]) + M[i][1] * L[4]) + M[i][2] * L[5] for i in range(3)]
    p0, p1 = C.fy * top[0], C.fx * top[1]
    p2 = (C.k20 * top[0] + C.k21 * top[1]) + C.k22 * top[2]
    den = _sqrt(p0 * p0 + p1 * p1)
    e0 = _div((xs * p0 + ys * p1) + p2, den)
    e1 = _div((xe * p0 + ye * p1) + p2, den)
    return e0 * (w * e0) + e1 * (w * e1), (e0, e1)


def perturbed(est):
    out = []
    for d in range(6):
        for v in (NUMERIC_DELTA, -NUMERIC_DELTA):
            u = [0.0] * 6
            u[d] = v
            out.append(oplus(u, est))
    return out


def line_terms(est, pert, C, L, xs, ys, xe, ye, w, robust, delta):
    scalar = 1.0 / (2.0 * NUMERIC_DELTA)
    J = [0.0] * 12
    for d in range(6):
        _, p = line_error(pert[2 * d], C, L, xs, ys, xe, ye, w)
        _, m = line_error(pert[2 * d + 1], C, L, xs, ys, xe, ye, w)
        J[d] = scalar * (p[0] - m[0])
        J[6 + d] = scalar * (p[1] - m[1])
    chi2, e = line_error(est, C, L, xs, ys, xe, ye, w)
    rho0, rho1 = huber(chi2, delta) if robust else (chi2, 1.0)
    return chi2, terms(J, 2, (e[0], e[1], 0.0), w, rho0, rho1)


# ---- item 4: the 6 x 6 solve
def h_index(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


def chol6(H21, b, lam):
    """(x, ok)"""
    Lf = [0.0] * 36
    x = [0.0] * 6
    y = [0.0] * 6
    for j in range(6):
        s = H21[h_index(j, j)] + lam
        for k in range(j):
            s = s - Lf[6 * j + k] * Lf[6 * j + k]
        if not (s > 0.0) or s > DBL_MAX:
            return [0.0] * 6, False
        d = math.sqrt(s)
        Lf[6 * j + j] = d
        for i in range(j + 1, 6):
            v = H21[h_index(j, i)]
            for k in range(j):
                v = v - Lf[6 * i + k] * Lf[6 * j + k]
            Lf[6 * i + j] = v / d
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - Lf[6 * i + k] * y[k]
        y[i] = v / Lf[6 * i + i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - Lf[6 * k + i] * x[k]
        x[i] = v / Lf[6 * i + i]
    return x, True


# ---- items 3, 5, 6: one frame
class Frame:
    """One frame in slot form.  points: list of dict(valid, x, y, octave, x_right, pos_w) per slot (x, y, x_right already f32 values);
    lines: list of dict(valid, sx, sy, ex, ey, octave, pos_w (6)) or None."""

    def __init__(self, cam, mono_setup, pose12, points, inv_sigma_sq, lines=None, inv_sigma_sq_lsd=()):
        self.cam, self.mono_setup, self.pose12 = cam, bool(mono_setup), [float(v) for v in pose12]
        self.points, self.lines = points, lines
        self.sig = [float(f32(v)) for v in inv_sigma_sq]
        self.sig_l = [float(f32(v)) for v in inv_sigma_sq_lsd]


def trial_robust(trial, num_trials):
    return num_trials < 2 or trial <= num_trials - 2


def _pass(F, est, pts, lns, level, llevel, chi2, lchi2, robust, lin):
    """one pass over the active edges in slot order, points before lines: the 28 sums (lin) or the robust chi2 alone in sums[27]"""
    delta_pt = DELTA_2D if F.mono_setup else DELTA_3D
    sums = [0.0] * 28
    pert = perturbed(est) if lin and lns else None
    for k, s in enumerate(pts):
        if level[k]:
            continue
        p = F.points[s]
        mono = p["x_right"] < 0.0
        w = F.sig[p["octave"]]
        if lin:
            chi2[k], T = point_terms(est, F.cam, p["pos_w"], p["x"], p["y"], p["x_right"], mono, w, robust, delta_pt)
            for t in range(28):
                sums[t] = sums[t] + T[t]
        else:
            chi2[k] = point_error(est, F.cam, p["pos_w"], p["x"], p["y"], p["x_right"], mono, w)[0]
            sums[27] = sums[27] + (huber(chi2[k], delta_pt)[0] if robust else chi2[k])
    for k, s in enumerate(lns):
        if llevel[k]:
            continue
        l = F.lines[s]
        w = F.sig_l[l["octave"]]
        if lin:
            lchi2[k], T = line_terms(est, pert, F.cam, l["pos_w"], l["sx"], l["sy"], l["ex"], l["ey"], w, robust, DELTA_2D)
            for t in range(28):
                sums[t] = sums[t] + T[t]
        else:
            lchi2[k] = line_error(est, F.cam, l["pos_w"], l["sx"], l["sy"], l["ex"], l["ey"], w)[0]
            sums[27] = sums[27] + (huber(lchi2[k], DELTA_2D)[0] if robust else lchi2[k])
    return sums


def linearize(F, robust=True, active=None, active_lines=None):
    """model_pose_linearize of one frame: (sums[28], {slot: chi2}, {line slot: chi2})"""
    pts = [s for s, p in enumerate(F.points) if p["valid"] and 0 <= p["octave"] < len(F.sig)]
    lns = [s for s, l in enumerate(F.lines or []) if l["valid"] and 0 <= l["octave"] < len(F.sig_l)]
    level = [0 if active is None or active[s] else 1 for s in pts]
    llevel = [0 if active_lines is None or active_lines[s] else 1 for s in lns]
    chi2, lchi2 = [NAN] * len(pts), [NAN] * len(lns)
    sums = _pass(F, est_from_pose(F.pose12), pts, lns, level, llevel, chi2, lchi2, robust, True)
    return sums, {s: chi2[k] for k, s in enumerate(pts) if not level[k]}, {s: lchi2[k] for k, s in enumerate(lns) if not llevel[k]}


def optimize(F, num_trials=4, num_each_iter=10, outlier=None, outlier_lines=None):
    """One frame.  outlier / outlier_lines: the caller's flag lists (values of slots that are not written stay).  Returns dict(status, pose (15),
    num_init_obs, num_valid, outlier, outlier_lines, trial_info, trial_chi2, stale_differs: the number of point / line flags over all trials
    that a fresh evaluation of an active edge at the kept estimate would have set differently)."""
    n_slots = len(F.points)
    l_slots = len(F.lines) if F.lines is not None else 0
    flags = list(outlier) if outlier is not None else [0] * n_slots
    lflags = list(outlier_lines) if outlier_lines is not None else [0] * l_slots
    info = [[0, 0, 0, 0] for _ in range(num_trials)]
    tchi = [[0.0, 0.0] for _ in range(num_trials)]
    pts = [s for s, p in enumerate(F.points) if p["valid"] and 0 <= p["octave"] < len(F.sig)]
    n = len(pts)
    for s in pts:
        flags[s] = 0
    res = dict(num_init_obs=n, outlier=flags, outlier_lines=lflags, trial_info=info, trial_chi2=tchi, stale_differs=0)
    if n < MIN_OBS:
        p = F.pose12
        cc = [((-p[i]) * p[9] + (-p[3 + i]) * p[10]) + (-p[6 + i]) * p[11] for i in range(3)]
        res.update(status=1, pose=list(p[:12]) + cc, num_valid=0)
        return res
    lns = [s for s, l in enumerate(F.lines or []) if l["valid"] and 0 <= l["octave"] < len(F.sig_l)]
    for s in lns:
        lflags[s] = 0
    level, llevel = [0] * n, [0] * len(lns)
    chi2, lchi2 = [0.0] * n, [0.0] * len(lns)
    est = est_from_pose(F.pose12)
    lam, ni, current_chi = 0.0, 2.0, 0.0
    num_bad = 0
    for trial in range(num_trials):
        robust = trial_robust(trial, num_trials)
        iterations = rejected = end = 0
        for it in range(num_each_iter):
            S = _pass(F, est, pts, lns, level, llevel, chi2, lchi2, robust, True)
            current_chi = S[27]
            if it == 0:
                m = 0.0
                for j in range(6):
                    d = abs(S[h_index(j, j)])
                    m = d if d > m else m
                lam = 1e-5 * m
                ni = 2.0
            qmax = 0
            rho = 0.0
            while True:
                bak = est
                x, ok2 = chol6(S[:21], S[21:27], lam)
                est = oplus(x, bak)
                temp_sum = _pass(F, est, pts, lns, level, llevel, chi2, lchi2, robust, False)[27]
                temp_chi = temp_sum if ok2 else DBL_MAX
                scale = 0.0
                for j in range(6):
                    scale = scale + x[j] * (lam * x[j] + S[21 + j])
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
        num_bad = 0
        for k, s in enumerate(pts):
            p = F.points[s]
            mono = p["x_right"] < 0.0
            fresh = point_error(est, F.cam, p["pos_w"], p["x"], p["y"], p["x_right"], mono, F.sig[p["octave"]])[0]
            c = fresh if level[k] else chi2[k]
            thr = CHI_SQ_2D if mono else CHI_SQ_3D
            bad = 1 if thr < c else 0
            res["stale_differs"] += int(bad != (1 if thr < fresh else 0))
            level[k] = bad
            flags[s] = bad
            num_bad += bad
        stop = n - num_bad < MIN_OBS
        if not stop:
            for k, s in enumerate(lns):
                l = F.lines[s]
                fresh = line_error(est, F.cam, l["pos_w"], l["sx"], l["sy"], l["ex"], l["ey"], F.sig_l[l["octave"]])[0]
                c = fresh if llevel[k] else lchi2[k]
                bad = 1 if CHI_SQ_2D < c else 0
                res["stale_differs"] += int(bad != (1 if CHI_SQ_2D < fresh else 0))
                llevel[k] = bad
                lflags[s] = bad
        info[trial] = [iterations, rejected, num_bad, end if end else END_ITERATIONS]
        tchi[trial] = [current_chi, lam]
        if stop:
            break
    res.update(status=0, pose=pose_from_est(est), num_valid=n - num_bad)
    return res
