"""Plain-Python restatement of DESIGN.md section 5, D28: optimize::local_bundle_adjuster_extended_line::optimize over map tables, written from that
paragraph.  What D28 takes from D17 (the sets of the points, the point edge's blocks, the landmark sums) is D17's restatement, tests/local_ba_ref.py,
and what it takes from D15 (the pose vertex, the line error, Huber, the pose block's 28 terms) is tests/pose_optimizer_ref.py; the line vertex, the
line edge's numeric Jacobian blocks, the mixed Schur solve and the line half of the schedule are here.  Python floats only (IEEE f64, one rounding per
operation, no fused multiply-add): the host build of csrc/local_ba_lines.hpp is held to this bit for bit (tests/test_local_ba_lines_cpu.py)."""
import local_ba_ref as REF
import pose_optimizer_ref as R15

DBL_MAX = R15.DBL_MAX
_div, _sqrt = R15._div, R15._sqrt
OK, NO_EDGES = REF.OK, REF.NO_EDGES
KF_NONE, KF_FREE, KF_ORIGIN, KF_FIXED = REF.KF_NONE, REF.KF_FREE, REF.KF_ORIGIN, REF.KF_FIXED
SCALAR = 1.0 / (2.0 * R15.NUMERIC_DELTA)


class LineTables:
    """the line tables beside a REF.Tables `points`: kls [F] lists of (xs, ys, xe, ye, octave), pluecker [LL][6], line_erased [LL], obs [LL] lists of
    (t, kf, idx) with t the entry's place in the lines' observation list, sigma the inv_level_sigma_sq_lsd list"""

    def __init__(self, points, sigma, kls, pluecker, obs, line_erased=None):
        self.points, self.sigma, self.kls, self.pluecker, self.obs = points, [float(s) for s in sigma], kls, pluecker, obs
        self.LL = len(pluecker)
        self.TL = sum(len(o) for o in obs)
        self.line_erased = line_erased or [0] * self.LL


# ---- the line vertex
def norm3(a, b, c):
    return _sqrt((a * a + b * b) + c * c)


def line_oplus(L, v):
    """Line3D::oplus: toOrthonormal, the update from v, the two products, fromOrthonormal and both normalize()"""
    m0, m1, m2, d0, d1, d2 = L
    dnorm, mnorm = norm3(d0, d1, d2), norm3(m0, m1, m2)
    wn = _div(1.0, _sqrt(dnorm * dnorm + mnorm * mnorm))
    W00, W01, W10, W11 = mnorm * wn, (-dnorm) * wn, dnorm * wn, mnorm * wn
    mn, dn = _div(1.0, mnorm), _div(1.0, dnorm)
    c0, c1, c2 = m1 * d2 - m2 * d1, m2 * d0 - m0 * d2, m0 * d1 - m1 * d0
    cn = _div(1.0, norm3(c0, c1, c2))
    U = [m0 * mn, d0 * dn, c0 * cn, m1 * mn, d1 * dn, c1 * cn, m2 * mn, d2 * dn, c2 * cn]
    sn, cs = R15.sincos(v[3])
    q = [v[0], v[1], v[2], _sqrt(1.0 - ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))]
    n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    if n2 > 0.0:
        n = _sqrt(n2)
        q = [_div(x, n) for x in q]
    Ru = R15.rot_from_quat(q)
    u0 = [(U[3 * i] * Ru[0] + U[3 * i + 1] * Ru[3]) + U[3 * i + 2] * Ru[6] for i in range(3)]
    u1 = [(U[3 * i] * Ru[1] + U[3 * i + 1] * Ru[4]) + U[3 * i + 2] * Ru[7] for i in range(3)]
    w0, w1 = W00 * cs + W01 * sn, W10 * cs + W11 * sn
    out = [u0[i] * w0 for i in range(3)] + [u1[i] * w1 for i in range(3)]
    for _ in range(2):
        n = _div(1.0, norm3(out[3], out[4], out[5]))
        out = [x * n for x in out]
    return out


def line_perturbed(L):
    out = []
    for d in range(4):
        for dv in (R15.NUMERIC_DELTA, -R15.NUMERIC_DELTA):
            v = [0.0] * 4
            v[d] = dv
            out.append(line_oplus(L, v))
    return out


def depth_ok(est, C, L, xs, ys, xe, ye):
    """depth_is_positive_via_endpoints_trimming at (est, L)"""
    R = R15.rot_from_quat(est)
    tx, ty, tz = est[4], est[5], est[6]
    M3 = [[(-tz) * R[3 + j] + ty * R[6 + j] for j in range(3)],
          [tz * R[j] + (-tx) * R[6 + j] for j in range(3)],
          [(-ty) * R[j] + tx * R[3 + j] for j in range(3)]]
    top = [((((R[3 * i] * L[0] + R[3 * i + 1] * L[1]) + R[3 * i + 2] * L[2]) + M3[i][0] * L[3]) + M3[i][1] * L[4]) + M3[i][2] * L[5] for i in range(3)]
    l1, l2 = C.fy * top[0], C.fx * top[1]
    l3 = (C.k20 * top[0] + C.k21 * top[1]) + C.k22 * top[2]
    den = l1 * l1 + l2 * l2
    Pm = [0.0] * 12
    for c in range(4):
        a0, a1, a2 = (R[c], R[3 + c], R[6 + c]) if c < 3 else (tx, ty, tz)
        Pm[c] = (C.fx * a0 + 0.0 * a1) + C.cx * a2
        Pm[4 + c] = (0.0 * a0 + C.fy * a1) + C.cy * a2
        Pm[8 + c] = (0.0 * a0 + 0.0 * a1) + 1.0 * a2
    M = [0.0, -L[2], L[1], L[3], L[2], 0.0, -L[0], L[4], -L[1], L[0], 0.0, L[5], -L[3], -L[4], -L[5], 0.0]

    def trim(x, y):
        xc = (-((y - _div(l2, l1) * x) + _div(l3, l2))) * _div(l1 * l2, den)
        yc = (-_div(l1, l2)) * xc - _div(l3, l2)
        y0 = y - _div(l2, l1) * x
        lt = [yc * 1.0 - 1.0 * y0, 1.0 * 0.0 - xc * 1.0, xc * y0 - yc * 0.0]
        pt = [(lt[0] * Pm[j] + lt[1] * Pm[4 + j]) + lt[2] * Pm[8 + j] for j in range(4)]
        I = [((M[4 * i] * pt[0] + M[4 * i + 1] * pt[1]) + M[4 * i + 2] * pt[2]) + M[4 * i + 3] * pt[3] for i in range(4)]
        return [_div(I[i], I[3]) for i in range(3)]

    sp, ep = trim(xs, ys), trim(xe, ye)
    zs = ((R[6] * sp[0] + R[7] * sp[1]) + R[8] * sp[2]) + tz * 1.0
    ze = ((R[6] * ep[0] + R[7] * ep[1]) + R[8] * ep[2]) + tz * 1.0
    return 0.0 < zs and 0.0 < ze


# ---- the 4 x 4 inverse
def h4(i, j):
    if i > j:
        i, j = j, i
    return i * 4 - (i * (i - 1)) // 2 + (j - i)


def chol4(H10, b, lam):
    """lev_chol at N = 4: (x, ok)"""
    N = 4
    Lf = [0.0] * 16
    x = [0.0] * N
    y = [0.0] * N
    for j in range(N):
        s = H10[h4(j, j)] + lam
        for k in range(j):
            s = s - Lf[N * j + k] * Lf[N * j + k]
        if not (s > 0.0) or s > DBL_MAX:
            return [0.0] * N, False
        d = _sqrt(s)
        Lf[N * j + j] = d
        for i in range(j + 1, N):
            v = H10[h4(j, i)]
            for k in range(j):
                v = v - Lf[N * i + k] * Lf[N * j + k]
            Lf[N * i + j] = _div(v, d)
    for i in range(N):
        v = b[i]
        for k in range(i):
            v = v - Lf[N * i + k] * y[k]
        y[i] = _div(v, Lf[N * i + i])
    for i in range(N - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, N):
            v = v - Lf[N * k + i] * x[k]
        x[i] = _div(v, Lf[N * i + i])
    return x, True


def inv4(H10, lam):
    """the upper triangle of (H + lambda I)^-1: column k from the solve against e_k, its rows 0 .. k; (inverse, ok)"""
    inv = [0.0] * 10
    ok = True
    for k in range(4):
        x, good = chol4(H10, [1.0 if i == k else 0.0 for i in range(4)], lam)
        ok = ok and good
        for i in range(k + 1):
            inv[h4(i, k)] = x[i]
    return inv, ok


class LEdge:
    def __init__(self, t, l, kf, xs, ys, xe, ye, w):
        self.t, self.l, self.kf, self.xs, self.ys, self.xe, self.ye, self.w = t, l, kf, xs, ys, xe, ye, w
        self.level, self.chi2, self.rho0 = 0, 0.0, 0.0


class Problem(REF.Problem):
    def __init__(self, LT, kf_local):
        Tb = LT.points
        REF.Problem.__init__(self, Tb, kf_local)
        self.LT = LT
        role = self.role
        self.ln_role = [0] * LT.LL
        for l in range(LT.LL):
            if not LT.line_erased[l]:
                self.ln_role[l] = int(any(0 <= kf < Tb.F and role[kf] in (KF_FREE, KF_ORIGIN) for _, kf, _ in LT.obs[l]))
        self.ledges = []
        fixed = set()
        for l in range(LT.LL):
            if not self.ln_role[l]:
                continue
            for t, kf, idx in LT.obs[l]:
                if not (0 <= kf < Tb.F) or Tb.kf_erased[kf]:
                    continue
                if role[kf] == KF_NONE:
                    fixed.add(kf)
                if not (0 <= idx < len(LT.kls[kf])):
                    continue
                xs, ys, xe, ye, octave = LT.kls[kf][idx]
                if not (0 <= octave < len(LT.sigma)):
                    continue
                self.ledges.append(LEdge(t, l, kf, float(xs), float(ys), float(xe), float(ye), LT.sigma[octave]))
        self.fixed_by_line_only = sorted(fixed)
        for f in fixed:
            role[f] = KF_FIXED
            self.kf_est[f] = R15.est_from_pose(Tb.pose[f][:12])
        self.ln_est = {l: [float(v) for v in LT.pluecker[l]] for l in range(LT.LL) if self.ln_role[l]}
        self.census = dict(failed_inv4=0, depth_only=0)      # what the tests ask about a run, not part of D28

    def round_setup(self):
        live = [e for e in self.edges if e.level == 0]
        llive = [e for e in self.ledges if e.level == 0]
        self.pa = [f for f in self.free if any(e.kf == f for e in live) or any(e.kf == f for e in llive)]
        self.la = sorted({e.l for e in live})
        self.na = sorted({e.l for e in llive})
        self.by_lm = {l: [e for e in live if e.l == l] for l in self.la}
        self.by_pose = {f: [e for e in live if e.kf == f] for f in self.pa}
        self.by_ln = {l: [e for e in llive if e.l == l] for l in self.na}
        self.by_pose_l = {f: [e for e in llive if e.kf == f] for f in self.pa}
        self.live, self.llive = live, llive

    def evaluate_all(self, kf_est, lm_est, ln_est, robust):
        total = self.evaluate(kf_est, lm_est, robust)
        C = self.Tb.cam
        for l in self.na:
            part = 0.0
            for e in self.by_ln[l]:
                chi2, _ = R15.line_error(kf_est[e.kf], C, ln_est[l], e.xs, e.ys, e.xe, e.ye, e.w)
                e.chi2 = chi2
                e.rho0 = R15.huber(chi2, R15.DELTA_2D)[0] if robust else chi2
                part = part + e.rho0
            total = total + part
        return total

    def linearize_all(self, robust):
        """the blocks at the kept estimates: D17's with the pose sums going on over the line edges, Hnn {l: 14}, Wn {t: 24}, the robust chi2"""
        C = self.Tb.cam
        Hpp, Hll, W, total = self.linearize(robust)
        pert = {f: R15.perturbed(self.kf_est[f]) for f in self.pa}
        lpert = {l: line_perturbed(self.ln_est[l]) for l in self.na}
        Hnn, Wn, T27 = {}, {}, {}
        for l in self.na:
            acc = [0.0] * 14
            part = 0.0
            Lc = self.ln_est[l]
            for e in self.by_ln[l]:
                est = self.kf_est[e.kf]
                obs = (e.xs, e.ys, e.xe, e.ye, e.w)
                chi2, err = R15.line_error(est, C, Lc, *obs)
                rho0, rho1 = R15.huber(chi2, R15.DELTA_2D) if robust else (chi2, 1.0)
                e.chi2, e.rho0 = chi2, rho0
                part = part + rho0
                free_pose = e.kf in self.by_pose
                Jp = [0.0] * 12
                if free_pose:
                    for d in range(6):
                        p = R15.line_error(pert[e.kf][2 * d], C, Lc, *obs)[1]
                        m = R15.line_error(pert[e.kf][2 * d + 1], C, Lc, *obs)[1]
                        Jp[d] = SCALAR * (p[0] - m[0])
                        Jp[6 + d] = SCALAR * (p[1] - m[1])
                Jl = [0.0] * 8
                for d in range(4):
                    p = R15.line_error(est, C, lpert[l][2 * d], *obs)[1]
                    m = R15.line_error(est, C, lpert[l][2 * d + 1], *obs)[1]
                    Jl[d] = SCALAR * (p[0] - m[0])
                    Jl[4 + d] = SCALAR * (p[1] - m[1])
                e.Jl = Jl
                wr = rho1 * e.w
                o = [(-(e.w * err[k])) * rho1 for k in range(2)]
                tl = [Jl[i] * (wr * Jl[j]) + Jl[4 + i] * (wr * Jl[4 + j]) for i in range(4) for j in range(i, 4)]
                tl += [Jl[i] * o[0] + Jl[4 + i] * o[1] for i in range(4)]
                acc = [a + b for a, b in zip(acc, tl)]
                if free_pose:
                    T27[e.t] = R15.terms(Jp, 2, (err[0], err[1], 0.0), e.w, rho0, rho1)[:27]
                    Wn[e.t] = [Jp[i] * (wr * Jl[j]) + Jp[6 + i] * (wr * Jl[4 + j]) for i in range(6) for j in range(4)]
            Hnn[l] = acc
            total = total + part
        for f in self.pa:
            acc = Hpp[f]
            for e in self.by_pose_l[f]:
                acc = [a + b for a, b in zip(acc, T27[e.t])]
            Hpp[f] = acc
        return Hpp, Hll, Hnn, W, Wn, total

    def optimize_all(self, iters, robust):
        iterations = rejected = end = 0
        current = 0.0
        if not self.la and not self.na:
            return 0, 0, 0, self.current, self.lam
        for it in range(iters):
            Hpp, Hll, Hnn, W, Wn, current = self.linearize_all(robust)
            if it == 0:
                self.start_chi.append(current)
                m = 0.0
                for f in self.pa:
                    for j in range(6):
                        d = abs(Hpp[f][R15.h_index(j, j)])
                        m = d if d > m else m
                for l in self.la:
                    for j in (0, 3, 5):
                        d = abs(Hll[l][j])
                        m = d if d > m else m
                for l in self.na:
                    for j in (0, 4, 7, 9):
                        d = abs(Hnn[l][j])
                        m = d if d > m else m
                self.lam, self.ni = 1e-5 * m, 2.0
            qmax, rho = 0, 0.0
            while True:
                ok, xp, xl, xn, bad4 = mixed_schur_solve(self.pa, self.la, self.na, self.by_pose, self.by_lm, self.by_pose_l, self.by_ln, Hpp, Hll, Hnn, W, Wn, self.lam)
                self.census["failed_inv4"] += bad4
                kf_try = dict(self.kf_est)
                for f in self.pa:
                    kf_try[f] = R15.oplus(xp[f], self.kf_est[f])
                lm_try = dict(self.lm_est)
                for l in self.la:
                    lm_try[l] = [self.lm_est[l][i] + xl[l][i] for i in range(3)]
                ln_try = dict(self.ln_est)
                for l in self.na:
                    ln_try[l] = line_oplus(self.ln_est[l], xn[l])
                temp = self.evaluate_all(kf_try, lm_try, ln_try, robust)
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
                for l in self.na:
                    part = 0.0
                    for i in range(4):
                        part = part + xn[l][i] * (self.lam * xn[l][i] + Hnn[l][10 + i])
                    scale = scale + part
                scale = scale + 1e-3
                rho = _div(current - temp_chi, scale)
                if rho > 0.0 and REF.finite(temp_chi):
                    v = 2.0 * rho - 1.0
                    alpha = 1.0 - (v * v) * v
                    alpha = alpha if alpha < 2.0 / 3.0 else 2.0 / 3.0
                    self.lam = self.lam * (alpha if alpha > 1.0 / 3.0 else 1.0 / 3.0)
                    self.ni = 2.0
                    current = temp_chi
                    self.kf_est, self.lm_est, self.ln_est = kf_try, lm_try, ln_try
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


def mixed_schur_solve(pa, la, na, by_pose, by_lm, by_pose_l, by_ln, Hpp, Hll, Hnn, W, Wn, lam):
    """one damped solve over 3- and 4-blocks: (ok, x_p {f: 6}, x_l {l: 3}, x_n {l: 4}, the number of failed 4 x 4 inverses)"""
    n = 6 * len(pa)
    idx = {f: i for i, f in enumerate(pa)}
    ok = True
    inv, invn = {}, {}
    bad4 = 0
    for l in la:
        a = list(Hll[l][:6])
        a[0] = a[0] + lam; a[3] = a[3] + lam; a[5] = a[5] + lam
        inv[l], good = REF.inv3(a)
        ok = ok and good
    for l in na:
        invn[l], good = inv4(Hnn[l][:10], lam)
        ok = ok and good
        bad4 += int(not good)
    S = [[0.0] * n for _ in range(n)]
    b = [0.0] * n
    for f in pa:
        i = idx[f]
        for r in range(6):
            for c in range(r, 6):
                S[6 * i + r][6 * i + c] = Hpp[f][R15.h_index(r, c)]
            S[6 * i + r][6 * i + r] = S[6 * i + r][6 * i + r] + lam
            b[6 * i + r] = Hpp[f][21 + r]
    Y, Yn = {}, {}
    for l in la:
        h = inv[l]
        for e in by_lm[l]:
            if e.kf in idx:
                w = W[e.t]
                Y[e.t] = [(w[3 * r] * h[REF.SYM3[0][k]] + w[3 * r + 1] * h[REF.SYM3[1][k]]) + w[3 * r + 2] * h[REF.SYM3[2][k]] for r in range(6) for k in range(3)]
    for l in na:
        h = invn[l]
        for e in by_ln[l]:
            if e.kf in idx:
                w = Wn[e.t]
                Yn[e.t] = [((w[4 * r] * h[h4(0, k)] + w[4 * r + 1] * h[h4(1, k)]) + w[4 * r + 2] * h[h4(2, k)]) + w[4 * r + 3] * h[h4(3, k)] for r in range(6) for k in range(4)]
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
        for ea in by_pose_l[f]:
            y = Yn[ea.t]
            hb = Hnn[ea.l]
            for r in range(6):
                b[6 * i + r] = b[6 * i + r] - (((y[4 * r] * hb[10] + y[4 * r + 1] * hb[11]) + y[4 * r + 2] * hb[12]) + y[4 * r + 3] * hb[13])
            for eb in by_ln[ea.l]:
                if eb.kf not in idx:
                    continue
                j = idx[eb.kf]
                if j < i:
                    continue
                wb = Wn[eb.t]
                for r in range(6):
                    for c in range(6):
                        if j == i and c < r:
                            continue
                        S[6 * i + r][6 * j + c] = S[6 * i + r][6 * j + c] - (((y[4 * r] * wb[4 * c] + y[4 * r + 1] * wb[4 * c + 1]) + y[4 * r + 2] * wb[4 * c + 2]) + y[4 * r + 3] * wb[4 * c + 3])
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
    xl, xn = {}, {}
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
        xl[l] = [(h[REF.SYM3[i][0]] * t3[0] + h[REF.SYM3[i][1]] * t3[1]) + h[REF.SYM3[i][2]] * t3[2] for i in range(3)]
    for l in na:
        if not ok:
            xn[l] = [0.0] * 4
            continue
        t4 = list(Hnn[l][10:14])
        for e in by_ln[l]:
            if e.kf not in idx:
                continue
            w, xs = Wn[e.t], xp[e.kf]
            for i in range(4):
                d = w[i] * xs[0]
                for r in range(1, 6):
                    d = d + w[4 * r + i] * xs[r]
                t4[i] = t4[i] - d
        h = invn[l]
        xn[l] = [((h[h4(i, 0)] * t4[0] + h[h4(i, 1)] * t4[1]) + h[h4(i, 2)] * t4[2]) + h[h4(i, 3)] * t4[3] for i in range(4)]
    return ok, xp, xl, xn, bad4


def line_is_outlier(P, e):
    deep = depth_ok(P.kf_est[e.kf], P.Tb.cam, P.ln_est[e.l], e.xs, e.ys, e.xe, e.ye)
    return R15.CHI_SQ_2D < e.chi2 or not deep


def optimize(LT, kf_local, num_first_iter=5, num_second_iter=10):
    """one problem: REF.optimize's dict and line_role, pluecker {l: 6}, outlier_lines {t: 0 / 1}"""
    P = Problem(LT, kf_local)
    Tb = LT.points
    if len(P.free) > REF.MAX_FREE:
        raise ValueError("more than 64 free key frames")
    out = dict(kf_role=P.role, lm_role=P.lm_role, line_role=P.ln_role, round_info=[[0] * 4, [0] * 4], round_chi2=[[0.0] * 2, [0.0] * 2], outlier={}, outlier_lines={},
               problem=P)
    if not P.edges and not P.ledges:
        out["status"] = NO_EDGES
        out["pose"] = {}
        for f in P.free:
            p = [float(v) for v in Tb.pose[f][:12]]
            out["pose"][f] = p + [((-p[i]) * p[9] + (-p[3 + i]) * p[10]) + (-p[6 + i]) * p[11] for i in range(3)]
        out["pos_w"] = {l: list(P.lm_est[l]) for l in P.lm_est}
        out["pluecker"] = {l: list(P.ln_est[l]) for l in P.ln_est}
        return out
    P.current, P.lam, P.ni = 0.0, 0.0, 2.0
    for rnd in range(2):
        P.round_setup()
        if rnd == 1:
            P.census["left_round_2"] = [l for l in P.ln_est if l not in P.na]
        its, rej, end, cur, lam = P.optimize_all(num_first_iter if rnd == 0 else num_second_iter, rnd == 0)
        drops = 0
        if rnd == 0:
            for e in P.edges:
                e.level = int(REF.is_outlier(P, e))
                drops += e.level
            for e in P.ledges:
                e.level = int(line_is_outlier(P, e))
                drops += e.level
                if e.level and not (R15.CHI_SQ_2D < e.chi2):
                    P.census["depth_only"] += 1
        out["round_info"][rnd] = [its, rej, drops, end if end else (R15.END_ITERATIONS if its else 0)]
        out["round_chi2"][rnd] = [P.current, P.lam]
    out["status"] = OK
    out["pose"] = {f: R15.pose_from_est(P.kf_est[f]) for f in P.free}
    out["pos_w"] = {l: list(P.lm_est[l]) for l in P.lm_est}
    out["pluecker"] = {l: list(P.ln_est[l]) for l in P.ln_est}
    out["outlier"] = {e.t: int(REF.is_outlier(P, e)) for e in P.edges}
    out["outlier_lines"] = {e.t: int(line_is_outlier(P, e)) for e in P.ledges}
    return out
