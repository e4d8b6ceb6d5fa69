"""Plain-Python restatement of DESIGN.md section 5, D17: optimize::local_bundle_adjuster::optimize over map tables, written from that paragraph.
What D17 takes from D15 (the vertex, exp, the point edge's error and pose Jacobian, Huber, the pose block's 28 terms) is D15's restatement,
tests/pose_optimizer_ref.py; everything else is here.  Python floats only (IEEE f64, one rounding per operation, no fused multiply-add): the
host build of csrc/local_ba.hpp is held to this bit for bit (tests/test_local_ba_cpu.py)."""
import pose_optimizer_ref as R15

DBL_MAX = R15.DBL_MAX
_div, _sqrt = R15._div, R15._sqrt
OK, NO_EDGES = 0, 1
KF_NONE, KF_FREE, KF_ORIGIN, KF_FIXED = 0, 1, 2, 3
MAX_FREE = 64


class Tables:
    """the map tables as Python values: pose [F][12], kf_erased, kf_is_origin [F], kps [F] lists of (x, y, octave, x_right), pos_w [L][3], lm_erased [L],
    obs [L] lists of (t, kf, idx) with t the entry's place in the observation list, cam an R15.Cam, sigma the inv_level_sigma_sq list, mono_setup"""

    def __init__(self, cam, mono_setup, sigma, pose, kps, pos_w, obs, kf_erased=None, kf_is_origin=None, lm_erased=None):
        self.cam, self.mono_setup, self.sigma, self.pose, self.kps, self.pos_w, self.obs = cam, bool(mono_setup), [float(s) for s in sigma], pose, kps, pos_w, obs
        self.F, self.L = len(pose), len(pos_w)
        self.T = sum(len(o) for o in obs)
        self.kf_erased = kf_erased or [0] * self.F
        self.kf_is_origin = kf_is_origin or [0] * self.F
        self.lm_erased = lm_erased or [0] * self.L


def finite(v):
    return -DBL_MAX <= v <= DBL_MAX


def inv3(a):
    """closed cofactor inverse of the symmetric (00 01 02 11 12 22); (inverse, ok)"""
    c00 = a[3] * a[5] - a[4] * a[4]; c01 = a[2] * a[4] - a[1] * a[5]; c02 = a[1] * a[4] - a[2] * a[3]
    c11 = a[0] * a[5] - a[2] * a[2]; c12 = a[1] * a[2] - a[0] * a[4]; c22 = a[0] * a[3] - a[1] * a[1]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    i = _div(1.0, det)
    o = [c00 * i, c01 * i, c02 * i, c11 * i, c12 * i, c22 * i]
    return o, all(finite(v) for v in o)


SYM3 = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]


class Edge:
    def __init__(self, t, l, kf, ox, oy, orr, w):
        self.t, self.l, self.kf, self.ox, self.oy, self.orr, self.w = t, l, kf, ox, oy, orr, w
        self.mono = orr < 0.0
        self.level, self.chi2, self.rho0 = 0, 0.0, 0.0


def sets(Tb, kf_local):
    """the roles and the edges in edge order: (kf_role [F], lm_role [L], edges)"""
    role = [KF_NONE] * Tb.F
    for f in range(Tb.F):
        if kf_local[f] and not Tb.kf_erased[f]:
            role[f] = KF_ORIGIN if Tb.kf_is_origin[f] else KF_FREE
    lm_role = [0] * Tb.L
    for l in range(Tb.L):
        if not Tb.lm_erased[l]:
            lm_role[l] = int(any(0 <= kf < Tb.F and role[kf] in (KF_FREE, KF_ORIGIN) for _, kf, _ in Tb.obs[l]))
    edges = []
    fixed = set()
    for l in range(Tb.L):
        if not lm_role[l]:
            continue
        for t, kf, idx in Tb.obs[l]:
            if not (0 <= kf < Tb.F) or Tb.kf_erased[kf]:
                continue
            if role[kf] == KF_NONE:
                fixed.add(kf)
            if not (0 <= idx < len(Tb.kps[kf])):
                continue
            x, y, octave, xr = Tb.kps[kf][idx]
            if not (0 <= octave < len(Tb.sigma)):
                continue
            edges.append(Edge(t, l, kf, float(x), float(y), float(xr), Tb.sigma[octave]))
    for f in fixed:
        role[f] = KF_FIXED
    return role, lm_role, edges


def lm_jacobian(C, est, pc, mono):
    x, y, z = pc
    z_sq = z * z
    Rm = R15.rot_from_quat(est)
    J = [0.0] * 9
    for c in range(3):
        J[c] = _div((-C.fx) * Rm[c], z) + _div((C.fx * x) * Rm[6 + c], z_sq)
        J[3 + c] = _div((-C.fy) * Rm[3 + c], z) + _div((C.fy * y) * Rm[6 + c], z_sq)
        J[6 + c] = J[c] - _div(C.fxb * Rm[6 + c], z_sq)
    return J


class Problem:
    def __init__(self, Tb, kf_local):
        self.Tb = Tb
        self.role, self.lm_role, self.edges = sets(Tb, kf_local)
        self.kf_est = {f: R15.est_from_pose(Tb.pose[f][:12]) for f in range(Tb.F) if self.role[f] != KF_NONE}
        self.lm_est = {l: [float(v) for v in Tb.pos_w[l]] for l in range(Tb.L) if self.lm_role[l]}
        self.free = [f for f in range(Tb.F) if self.role[f] == KF_FREE]
        self.delta = R15.DELTA_2D if Tb.mono_setup else R15.DELTA_3D
        self.start_chi, self.thetas = [], []                 # what the tests ask about a run, not part of D17

    def round_setup(self):
        """the active sets of a round: free key frames and landmarks with a level-0 edge, in table order"""
        live = [e for e in self.edges if e.level == 0]
        self.pa = [f for f in self.free if any(e.kf == f for e in live)]
        self.la = sorted({e.l for e in live})
        self.by_lm = {l: [e for e in live if e.l == l] for l in self.la}
        self.by_pose = {f: [e for e in live if e.kf == f] for f in self.pa}
        self.live = live

    def evaluate(self, kf_est, lm_est, robust):
        """errors at the given estimates: every level-0 edge's chi2 and rho0; returns the robust sum (per landmark, then over the landmarks)"""
        total = 0.0
        for l in self.la:
            part = 0.0
            for e in self.by_lm[l]:
                chi2, _, _ = R15.point_error(kf_est[e.kf], self.Tb.cam, lm_est[l], e.ox, e.oy, e.orr, e.mono, e.w)
                e.chi2 = chi2
                e.rho0 = R15.huber(chi2, self.delta)[0] if robust else chi2
                part = part + e.rho0
            total = total + part
        return total

    def linearize(self, robust):
        """the blocks at the kept estimates: Hpp {f: 27}, Hll {l: 9}, W {t: 18}, and the robust chi2"""
        C = self.Tb.cam
        Hll, W, T27 = {}, {}, {}
        total = 0.0
        for l in self.la:
            acc = [0.0] * 9
            part = 0.0
            for e in self.by_lm[l]:
                est = self.kf_est[e.kf]
                chi2, pc, err = R15.point_error(est, C, self.lm_est[l], e.ox, e.oy, e.orr, e.mono, e.w)
                rho0, rho1 = R15.huber(chi2, self.delta) if robust else (chi2, 1.0)
                e.chi2, e.rho0 = chi2, rho0
                part = part + rho0
                Jp = R15.point_jacobian(C, pc)
                Jl = lm_jacobian(C, est, pc, e.mono)
                rows = 2 if e.mono else 3
                wr = rho1 * e.w
                o = [(-(e.w * err[k])) * rho1 for k in range(3)]
                tl = []
                for i in range(3):
                    for j in range(i, 3):
                        v = Jl[i] * (wr * Jl[j]) + Jl[3 + i] * (wr * Jl[3 + j])
                        if rows == 3:
                            v = v + Jl[6 + i] * (wr * Jl[6 + j])
                        tl.append(v)
                for i in range(3):
                    v = Jl[i] * o[0] + Jl[3 + i] * o[1]
                    if rows == 3:
                        v = v + Jl[6 + i] * o[2]
                    tl.append(v)
                acc = [a + b for a, b in zip(acc, tl)]
                if e.kf in self.by_pose:
                    T27[e.t] = R15.terms(Jp, rows, err, e.w, rho0, rho1)[:27]
                    w18 = []
                    for i in range(6):
                        for j in range(3):
                            v = Jp[i] * (wr * Jl[j]) + Jp[6 + i] * (wr * Jl[3 + j])
                            if rows == 3:
                                v = v + Jp[12 + i] * (wr * Jl[6 + j])
                            w18.append(v)
                    W[e.t] = w18
            Hll[l] = acc
            total = total + part
        Hpp = {}
        for f in self.pa:
            acc = [0.0] * 27
            for e in self.by_pose[f]:
                acc = [a + b for a, b in zip(acc, T27[e.t])]
            Hpp[f] = acc
        return Hpp, Hll, W, total

    def solve(self, Hpp, Hll, W, lam):
        return schur_solve(self.pa, self.la, self.by_pose, self.by_lm, Hpp, Hll, W, lam)

    def optimize(self, iters, robust):
        """g2o's optimize(iters) on the active sets: (iterations, rejected, end, current_chi, lambda)"""
        iterations = rejected = end = 0
        current = lam = 0.0
        if not self.la:
            return 0, 0, 0, self.current, self.lam
        for it in range(iters):
            Hpp, Hll, W, current = self.linearize(robust)
            if it == 0:
                self.start_chi.append(current)               # the chi2 a round starts from (tests/test_local_ba_cpu.py, anchor (f))
                m = 0.0
                for f in self.pa:
                    for j in range(6):
                        d = abs(Hpp[f][R15.h_index(j, j)])
                        m = d if d > m else m
                for l in self.la:
                    for j in (0, 3, 5):
                        d = abs(Hll[l][j])
                        m = d if d > m else m
                self.lam, self.ni = 1e-5 * m, 2.0
            lam = self.lam
            qmax, rho = 0, 0.0
            while True:
                ok, xp, xl = self.solve(Hpp, Hll, W, self.lam)
                kf_try = dict(self.kf_est)
                for f in self.pa:
                    kf_try[f] = R15.oplus(xp[f], self.kf_est[f])
                    self.thetas.append(_sqrt((xp[f][0] * xp[f][0] + xp[f][1] * xp[f][1]) + xp[f][2] * xp[f][2]))   # which branch of exp the update took
                lm_try = dict(self.lm_est)
                for l in self.la:
                    lm_try[l] = [self.lm_est[l][i] + xl[l][i] for i in range(3)]
                temp = self.evaluate(kf_try, lm_try, robust)
                temp_chi = temp if ok else DBL_MAX
                scale = 0.0
                for f in self.pa:
                    part = 0.0
                    for i in range(6):
                        part = part + xp[f][i] * (self.lam * xp[f][i] + Hpp[f][21 + i])
                    scale = scale + part
                for l in self.la:
                    part = 0.0
                    for i in range(3):
                        part = part + xl[l][i] * (self.lam * xl[l][i] + Hll[l][6 + i])
                    scale = scale + part
                scale = scale + 1e-3
                rho = _div(current - temp_chi, scale)
                if rho > 0.0 and finite(temp_chi):
                    v = 2.0 * rho - 1.0
                    alpha = 1.0 - (v * v) * v
                    alpha = alpha if alpha < 2.0 / 3.0 else 2.0 / 3.0
                    self.lam = self.lam * (alpha if alpha > 1.0 / 3.0 else 1.0 / 3.0)
                    self.ni = 2.0
                    current = temp_chi
                    self.kf_est, self.lm_est = kf_try, lm_try
                else:
                    self.lam = self.lam * self.ni
                    self.ni = self.ni * 2.0
                    rejected += 1
                qmax += 1
                if not (rho < 0.0 and qmax < R15.MAX_TRIES):
                    break
            iterations += 1
            end = R15.END_TRIES if qmax == R15.MAX_TRIES else R15.END_RHO_ZERO if rho == 0.0 else 0
            self.current = current
            if end:
                break
        return iterations, rejected, end, current, self.lam


def schur_solve(pa, la, by_pose, by_lm, Hpp, Hll, W, lam):
    """one damped solve: (ok, x_p {f: 6}, x_l {l: 3}); every x is zero when a 3 x 3 inverse or a pivot fails"""
    n = 6 * len(pa)
    idx = {f: i for i, f in enumerate(pa)}
    ok = True
    inv = {}
    for l in la:
        a = list(Hll[l][:6])
        a[0] = a[0] + lam; a[3] = a[3] + lam; a[5] = a[5] + lam
        inv[l], good = inv3(a)
        ok = ok and good
    S = [[0.0] * n for _ in range(n)]
    b = [0.0] * n
    for f in pa:
        i = idx[f]
        for r in range(6):
            for c in range(r, 6):
                S[6 * i + r][6 * i + c] = Hpp[f][R15.h_index(r, c)]
            S[6 * i + r][6 * i + r] = S[6 * i + r][6 * i + r] + lam
            b[6 * i + r] = Hpp[f][21 + r]
    Y = {}
    for l in la:
        h = inv[l]
        for e in by_lm[l]:
            if e.kf in idx:
                w = W[e.t]
                Y[e.t] = [(w[3 * r] * h[SYM3[0][k]] + w[3 * r + 1] * h[SYM3[1][k]]) + w[3 * r + 2] * h[SYM3[2][k]] for r in range(6) for k in range(3)]
    for f in pa:
        i = idx[f]
        for ea in by_pose[f]:
            y = Y[ea.t]
            for r in range(6):
                b[6 * i + r] = b[6 * i + r] - ((y[3 * r] * Hll[ea.l][6] + y[3 * r + 1] * Hll[ea.l][7]) + y[3 * r + 2] * Hll[ea.l][8])
            for eb in by_lm[ea.l]:
                if eb.kf not in idx:
                    continue
                j = idx[eb.kf]
                if j < i:
                    continue
                wb = W[eb.t]
                for r in range(6):
                    for c in range(6):
                        if j == i and c < r:
                            continue
                        S[6 * i + r][6 * j + c] = S[6 * i + r][6 * j + c] - ((y[3 * r] * wb[3 * c] + y[3 * r + 1] * wb[3 * c + 1]) + y[3 * r + 2] * wb[3 * c + 2])
    # Cholesky of the upper triangle, column by column; forward substitution with k ascending, back substitution with k descending
    Lf = [[0.0] * n for _ in range(n)]
    for j in range(n):
        if not ok:
            break
        s = S[j][j]
        for k in range(j):
            s = s - Lf[j][k] * Lf[j][k]
        if not (s > 0.0) or s > DBL_MAX:
            ok = False
            break
        d = _sqrt(s)
        Lf[j][j] = d
        for p in range(j + 1, n):
            v = S[j][p]
            for k in range(j):
                v = v - Lf[p][k] * Lf[j][k]
            Lf[p][j] = _div(v, d)
    x = [0.0] * n
    if ok:
        yv = [0.0] * n
        for i in range(n):
            v = b[i]
            for k in range(i):
                v = v - Lf[i][k] * yv[k]
            yv[i] = _div(v, Lf[i][i])
        for i in range(n - 1, -1, -1):
            v = yv[i]
            for k in range(n - 1, i, -1):
                v = v - Lf[k][i] * x[k]
            x[i] = _div(v, Lf[i][i])
    xp = {f: x[6 * idx[f]:6 * idx[f] + 6] for f in pa}
    xl = {}
    for l in la:
        if not ok:
            xl[l] = [0.0, 0.0, 0.0]
            continue
        t3 = list(Hll[l][6:9])
        for e in by_lm[l]:
            if e.kf not in idx:
                continue
            w, xs = W[e.t], xp[e.kf]
            for i in range(3):
                d = w[i] * xs[0]
                for r in range(1, 6):
                    d = d + w[3 * r + i] * xs[r]
                t3[i] = t3[i] - d
        h = inv[l]
        xl[l] = [(h[SYM3[i][0]] * t3[0] + h[SYM3[i][1]] * t3[1]) + h[SYM3[i][2]] * t3[2] for i in range(3)]
    return ok, xp, xl


def is_outlier(P, e):
    z = R15.se3_map(P.kf_est[e.kf], P.lm_est[e.l])[2]
    thr = R15.CHI_SQ_2D if e.mono else R15.CHI_SQ_3D
    return thr < e.chi2 or not (0.0 < z)


def optimize(Tb, kf_local, num_first_iter=5, num_second_iter=10):
    """one problem: dict(status, kf_role, lm_role, pose {f: 15}, pos_w {l: 3}, outlier {t: 0 / 1}, round_info [2][4], round_chi2 [2][2], census)"""
    P = Problem(Tb, kf_local)
    if len(P.free) > MAX_FREE:
        raise ValueError("more than 64 free key frames")
    out = dict(kf_role=P.role, lm_role=P.lm_role, round_info=[[0] * 4, [0] * 4], round_chi2=[[0.0] * 2, [0.0] * 2], outlier={})
    if not P.edges:
        out["status"] = NO_EDGES
        out["pose"] = {}
        for f in P.free:
            p = [float(v) for v in Tb.pose[f][:12]]
            out["pose"][f] = p + [((-p[i]) * p[9] + (-p[3 + i]) * p[10]) + (-p[6 + i]) * p[11] for i in range(3)]
        out["pos_w"] = {l: list(P.lm_est[l]) for l in P.lm_est}
        return out
    P.current, P.lam, P.ni = 0.0, 0.0, 2.0
    for rnd in range(2):
        P.round_setup()
        its, rej, end, cur, lam = P.optimize(num_first_iter if rnd == 0 else num_second_iter, rnd == 0)
        drops = 0
        if rnd == 0:
            for e in P.edges:
                e.level = int(is_outlier(P, e))
                drops += e.level
        out["round_info"][rnd] = [its, rej, drops, end if end else (R15.END_ITERATIONS if its else 0)]
        out["round_chi2"][rnd] = [P.current, P.lam]
    out["status"] = OK
    out["pose"] = {f: R15.pose_from_est(P.kf_est[f]) for f in P.free}
    out["pos_w"] = {l: list(P.lm_est[l]) for l in P.lm_est}
    out["outlier"] = {e.t: int(is_outlier(P, e)) for e in P.edges}
    out["problem"] = P
    return out
