"""A plain-Python restatement of solve::pnp_solver (src/PLPSLAM/solve/pnp_solver.cc:36-866) and of DESIGN.md section 5, D14, written from
those two texts: Python floats (IEEE f64), math.sqrt, lists.  It shares no code with the library; tests/test_pnp_solver_cpu.py holds the host
build of csrc/pnp.hpp to it bit for bit.

`linalg` swaps the four Jacobi uses for other routines (tests/test_pnp_solver_cpu.py passes numpy's svd / lstsq there: the stand-in for an
Eigen build, not the code under test)."""
import math
import struct

SWEEP_LIMIT = 60
SKIP_TOL = 2.0 ** -100
INF = float("inf")


# ---- float (f32) arithmetic: a product, sum or quotient of two floats rounded once from its f64 value equals the float operation
def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def ref_cos(v):
    """util::cos (util/trigonometric.h:42-73)"""
    PI = f32(3.14159265358979)
    PI_2 = f32(PI / 2.0)
    TWO_PI = f32(2.0 * PI)
    INV_TWO_PI = f32(1.0 / TWO_PI)
    THREE_PI_2 = f32(3.0 * PI_2)

    def poly(v):
        c1, c2, c3 = f32(0.99940307), f32(-0.49558072), f32(0.03679168)
        v2 = f32(v * v)
        return f32(c1 + f32(v2 * f32(c2 + f32(c3 * v2))))

    q = f32(v * INV_TWO_PI)
    fl = int(q)                      # cvFloor: (int) truncates, minus one when that is above the value
    if fl > q:
        fl -= 1
    v = f32(v - f32(f32(float(fl)) * TWO_PI))
    v = v if 0.0 < v else -v
    if v < PI_2:
        return poly(v)
    if v < PI:
        return -poly(f32(PI - v))
    if v < THREE_PI_2:
        return -poly(f32(v - PI))
    return poly(f32(TWO_PI - v))


def thresholds(scale_factors):
    """max_cos_errors_ per level (:47-51)"""
    max_rad_error = 1.0 * math.pi / 180.0
    return [ref_cos(f32(f32(s) * max_rad_error)) for s in scale_factors]


# ---- D14 item 1: the one-sided Jacobi
def partner(j, r, N):
    if j == N - 1:
        return r
    if j == r:
        return N - 1
    return (2 * r - j) % (N - 1)


def hestenes(G, V):
    """G: list of n columns of m numbers, V: list of n columns of n numbers (the identity); both rotated in place.  Returns the sweeps that
    rotated."""
    n = len(G)
    m = len(G[0]) if n else 0
    N = n + (n & 1)
    sweeps = 0
    while sweeps < SWEEP_LIMIT:
        rotated = False
        for r in range(N - 1):
            for p in range(n):
                q = partner(p, r, N)
                if q >= n or q < p:
                    continue
                gp, gq = G[p], G[q]
                alpha = beta = gamma = 0.0
                for i in range(m):
                    alpha = alpha + gp[i] * gp[i]
                    beta = beta + gq[i] * gq[i]
                    gamma = gamma + gp[i] * gq[i]
                if not (gamma * gamma > SKIP_TOL * (alpha * beta)):
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                root = math.sqrt(1.0 + zeta * zeta)
                t = 1.0 / (zeta + root) if zeta >= 0.0 else -1.0 / (root - zeta)
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                rotated = True
                for cols, k in ((G, m), (V, n)):
                    a, b = cols[p], cols[q]
                    for i in range(k):
                        x, y = a[i], b[i]
                        a[i] = c * x - s * y
                        b[i] = s * x + c * y
        if not rotated:
            break
        sweeps += 1
    return sweeps


def identity(n):
    return [[1.0 if i == j else 0.0 for i in range(n)] for j in range(n)]


def norm2(col):
    acc = 0.0
    for x in col:
        acc = acc + x * x
    return acc


def ranks(keys):
    """position of every column when the keys (NaN = +inf) are sorted descending, equal keys by ascending column"""
    keys = [k if k == k else INF for k in keys]
    return [sum(1 for k in range(len(keys)) if keys[k] > keys[j] or (keys[k] == keys[j] and k < j)) for j in range(len(keys))], keys


def sym_jacobi(A):
    """uses 1 and 2: A symmetric n x n (rows).  Returns (vals descending, Ut rows, sweeps)."""
    n = len(A)
    G = [[A[i][j] for i in range(n)] for j in range(n)]
    V = identity(n)
    sweeps = hestenes(G, V)
    rk, keys = ranks([norm2(g) for g in G])
    vals, Ut = [0.0] * n, [None] * n
    for j in range(n):
        vals[rk[j]] = math.sqrt(keys[j])
        Ut[rk[j]] = list(V[j])
    return vals, Ut, sweeps


def lstsq6(A, b):
    """use 3: A 6 x k (rows), b 6.  Returns (x, sweeps)."""
    k = len(A[0])
    G = [[A[i][j] for i in range(6)] for j in range(k)]
    V = identity(k)
    sweeps = hestenes(G, V)
    n2 = [norm2(g) for g in G]
    smax = 0.0
    for v in n2:
        sg = math.sqrt(v) if v >= 0.0 else float("nan")
        if sg > smax:
            smax = sg
    thr = (float(k) * 2.0 ** -52) * smax
    x = [0.0] * k
    for j in range(k):
        sg = math.sqrt(n2[j]) if n2[j] >= 0.0 else float("nan")
        if not (sg > thr):
            continue
        gb = 0.0
        for i in range(6):
            gb = gb + G[j][i] * b[i]
        coef = gb / n2[j]
        for i in range(k):
            x[i] = x[i] + V[j][i] * coef
    return x, sweeps


def rot_from_abt(Abt):
    """use 4: Abt 3 x 3 (rows).  Returns (R rows, sweeps)."""
    G = [[Abt[i][j] for i in range(3)] for j in range(3)]
    V = identity(3)
    sweeps = hestenes(G, V)
    rk, keys = ranks([norm2(g) for g in G])
    jmin = rk.index(2)
    U = []
    for j in range(3):
        sg = math.sqrt(keys[j])
        have = sg > 0.0 and sg < INF
        U.append([G[j][i] / sg if have else 0.0 for i in range(3)])
    sg = math.sqrt(keys[jmin])
    if not (sg > 0.0 and sg < INF):
        a = 1 if jmin == 0 else 0
        b = 1 if jmin == 2 else 2
        ua, ub = U[a], U[b]
        U[jmin] = [ua[1] * ub[2] - ua[2] * ub[1], ua[2] * ub[0] - ua[0] * ub[2], ua[0] * ub[1] - ua[1] * ub[0]]

    def product():
        return [[(U[0][i] * V[0][j] + U[1][i] * V[1][j]) + U[2][i] * V[2][j] for j in range(3)] for i in range(3)]

    R = product()
    det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0]
           - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
    if det < 0:
        V[jmin] = [-x for x in V[jmin]]
        R = product()
    return R, sweeps


class Jacobi:
    """the four uses as D14 defines them"""
    sym = staticmethod(sym_jacobi)
    lstsq = staticmethod(lstsq6)
    rot = staticmethod(rot_from_abt)


# ---- EPnP (:204-866)
def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(a, b):
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2])


def correspondences(pos_w, bearing):
    """add_correspondence (:204-228) over the lists: (pws, us, signs)"""
    pws, us, signs = [], [], []
    for w, b in zip(pos_w, bearing):
        if b[2] == 0:
            continue
        pws.append([w[0], w[1], w[2]])
        us.append([b[0] / b[2], b[1] / b[2]])
        signs.append(1 if 0.0 < b[2] else -1)
    return pws, us, signs


def qr_solve(A, b, X):
    """:748-866 on the row-major copy pA of the 6 x 4 matrix; X keeps its values on the early return"""
    nr, nc = 6, 4
    pA = [A[i][j] for i in range(6) for j in range(4)]
    A1, A2 = [0.0] * nr, [0.0] * nr
    kk = 0
    for k in range(nc):
        ik = kk
        eta = abs(pA[ik])
        for i in range(k + 1, nr):
            elt = abs(pA[ik])
            if eta < elt:
                eta = elt
            ik += nc
        if eta == 0:
            return
        ik = kk
        s = 0.0
        inv_eta = div(1.0, eta)
        for i in range(k, nr):
            pA[ik] *= inv_eta
            s += pA[ik] * pA[ik]
            ik += nc
        sigma = sqrt_(s)
        if pA[kk] < 0:
            sigma = -sigma
        pA[kk] += sigma
        A1[k] = sigma * pA[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            ik = kk
            s = 0.0
            for i in range(k, nr):
                s += pA[ik] * pA[ik + j - k]
                ik += nc
            tau = div(s, A1[k])
            ik = kk
            for i in range(k, nr):
                pA[ik + j - k] -= tau * pA[ik]
                ik += nc
        kk += nc + 1
    jj = 0
    for j in range(nc):
        ij = jj
        tau = 0.0
        for i in range(j, nr):
            tau += pA[ij] * b[i]
            ij += nc
        tau = div(tau, A1[j])
        ij = jj
        for i in range(j, nr):
            b[i] -= tau * pA[ij]
            ij += nc
        jj += nc + 1
    X[nc - 1] = div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        ij = i * nc + (i + 1)
        s = 0.0
        for j in range(i + 1, nc):
            s += pA[ij] * X[j]
            ij += 1
        X[i] = div(b[i] - s, A2[i])


def gauss_newton(L, rho, betas):
    """:728-746 with :714-726"""
    X = [0.0] * 4
    for _ in range(5):
        A, B = [], []
        for i in range(6):
            l = L[i]
            A.append([2 * l[0] * betas[0] + l[1] * betas[1] + l[3] * betas[2] + l[6] * betas[3],
                      l[1] * betas[0] + 2 * l[2] * betas[1] + l[4] * betas[2] + l[7] * betas[3],
                      l[3] * betas[0] + l[4] * betas[1] + 2 * l[5] * betas[2] + l[8] * betas[3],
                      l[6] * betas[0] + l[7] * betas[1] + l[8] * betas[2] + 2 * l[9] * betas[3]])
            B.append(rho[i] - (l[0] * betas[0] * betas[0] + l[1] * betas[0] * betas[1] + l[2] * betas[1] * betas[1] + l[3] * betas[0] * betas[2]
                               + l[4] * betas[1] * betas[2] + l[5] * betas[2] * betas[2] + l[6] * betas[0] * betas[3] + l[7] * betas[1] * betas[3]
                               + l[8] * betas[2] * betas[3] + l[9] * betas[3] * betas[3]))
        qr_solve(A, B, X)
        for i in range(4):
            betas[i] += X[i]


def inverse3(CC):
    """CC.inverse() as D14 defines it: cyclic cofactors, det along the first column, times 1 / det"""
    cof = [[CC[(r + 1) % 3][(c + 1) % 3] * CC[(r + 2) % 3][(c + 2) % 3] - CC[(r + 1) % 3][(c + 2) % 3] * CC[(r + 2) % 3][(c + 1) % 3] for c in range(3)]
           for r in range(3)]
    det = (cof[0][0] * CC[0][0] + cof[1][0] * CC[1][0]) + cof[2][0] * CC[2][0]
    invdet = div(1.0, det)
    return [[cof[j][i] * invdet for j in range(3)] for i in range(3)]


def canonical_sign(v):
    """D14 item 2a: the sign of a singular vector is the routine's own affair; the component of largest magnitude (the first of equals) is
    made non-negative"""
    big = 0
    for i in range(1, len(v)):
        if abs(v[i]) > abs(v[big]):
            big = i
    return [-x for x in v] if v[big] < 0 else list(v)


def canonical_basis(null):
    """D14 item 2a: with at most four correspondences M has at most eight rows, the four vectors span nothing but null space, and which basis
    of it a routine returns is its own affair.  The basis used is made a function of the span alone: column c of the projector
    sum_k n_k n_k^T, c = 0 .. 3, orthogonalised against the earlier ones (modified Gram-Schmidt) and scaled to unit length."""
    out = []
    for c in range(4):
        w = []
        for i in range(12):
            acc = 0.0
            for k in range(4):
                acc = acc + null[k][i] * null[k][c]
            w.append(acc)
        for b in out:
            d = 0.0
            for i in range(12):
                d = d + b[i] * w[i]
            for i in range(12):
                w[i] = w[i] - d * b[i]
        n2 = 0.0
        for i in range(12):
            n2 = n2 + w[i] * w[i]
        nrm = sqrt_(n2)
        out.append([div(w[i], nrm) for i in range(12)])
    return out


def compute_pose(pos_w, bearing, linalg=Jacobi, trace=None):
    """:230-290 for the correspondences the lists give.  Returns dict(R rows, t, err, N 1 .. 3, sweeps of the eight Jacobi uses), or None when
    add_correspondence keeps none.  trace: a dict of lists that receives the matrices the four Jacobi uses see (S3, MtM, L6 = (A, rho), Abt)."""
    def note(key, value):
        if trace is not None:
            trace.setdefault(key, []).append(value)

    pws, us, signs = correspondences(pos_w, bearing)
    nc = len(pws)
    if nc == 0:
        return None
    fnc = float(nc)
    sweeps = [0] * 8
    # choose_control_points (:292-333)
    cws = [[0.0, 0.0, 0.0] for _ in range(4)]
    for i in range(nc):
        for j in range(3):
            cws[0][j] += pws[i][j]
    for j in range(3):
        cws[0][j] /= fnc
    S3 = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            acc = 0.0
            for i in range(nc):
                acc = acc + (pws[i][a] - cws[0][a]) * (pws[i][b] - cws[0][b])
            S3[a][b] = S3[b][a] = acc
    note("S3", [list(r) for r in S3])
    D, Ut3, sweeps[0] = linalg.sym(S3)
    Ut3 = [canonical_sign(row) for row in Ut3]
    for i in range(1, 4):
        k = sqrt_(D[i - 1] / fnc)
        for j in range(3):
            cws[i][j] = cws[0][j] + k * Ut3[i - 1][j]
    # compute_barycentric_coordinates (:335-361)
    CC = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    CCi = inverse3(CC)
    alphas = []
    for p in pws:
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = CCi[j][0] * (p[0] - cws[0][0]) + CCi[j][1] * (p[1] - cws[0][1]) + CCi[j][2] * (p[2] - cws[0][2])
        a[0] = 1.0 - a[1] - a[2] - a[3]
        alphas.append(a)
    # fill_M (:363-375) with fx_ = fy_ = 1, cx_ = cy_ = 0, and M^T M: every entry one accumulator over the rows of M in ascending order
    M = []
    for a, (u, v) in zip(alphas, us):
        r0, r1 = [], []
        for i in range(4):
            r0 += [a[i] * 1.0, 0.0, a[i] * (0.0 - u)]
            r1 += [0.0, a[i] * 1.0, a[i] * (0.0 - v)]
        M += [r0, r1]
    MtM = [[0.0] * 12 for _ in range(12)]
    for a in range(12):
        for b in range(a, 12):
            acc = 0.0
            for row in M:
                acc = acc + row[a] * row[b]
            MtM[a][b] = MtM[b][a] = acc
    note("MtM", [list(r) for r in MtM])
    _, Ut, sweeps[1] = linalg.sym(MtM)
    null = [Ut[11 - i] for i in range(4)]
    if nc <= 4:
        null = canonical_basis(null)
    # compute_L_6x10 (:667-702), compute_rho (:704-712)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = [[[null[i][3 * a + k] - null[i][3 * b + k] for k in range(3)] for (a, b) in pairs] for i in range(4)]
    L = []
    for i in range(6):
        L.append([dot3(dv[0][i], dv[0][i]), 2.0 * dot3(dv[0][i], dv[1][i]), dot3(dv[1][i], dv[1][i]), 2.0 * dot3(dv[0][i], dv[2][i]),
                  2.0 * dot3(dv[1][i], dv[2][i]), dot3(dv[2][i], dv[2][i]), 2.0 * dot3(dv[0][i], dv[3][i]), 2.0 * dot3(dv[1][i], dv[3][i]),
                  2.0 * dot3(dv[2][i], dv[3][i]), dot3(dv[3][i], dv[3][i])])
    rho = [dist2(cws[a], cws[b]) for (a, b) in pairs]
    # find_betas_approx_1 .. 3 (:558-665)
    Betas = []
    note("L6", ([[l[0], l[1], l[3], l[6]] for l in L], list(rho)))
    b4, sweeps[2] = linalg.lstsq([[l[0], l[1], l[3], l[6]] for l in L], rho)
    if b4[0] < 0:
        b0 = math.sqrt(-b4[0])
        Betas.append([b0, div(-b4[1], b0), div(-b4[2], b0), div(-b4[3], b0)])
    else:
        b0 = math.sqrt(b4[0])
        Betas.append([b0, div(b4[1], b0), div(b4[2], b0), div(b4[3], b0)])
    for cols, slot in (((0, 1, 2), 3), ((0, 1, 2, 3, 4), 4)):
        note("L6", ([[l[c] for c in cols] for l in L], list(rho)))
        x, sweeps[slot] = linalg.lstsq([[l[c] for c in cols] for l in L], rho)
        if x[0] < 0:
            b0 = math.sqrt(-x[0])
            b1 = math.sqrt(-x[2]) if x[2] < 0 else 0.0
        else:
            b0 = math.sqrt(x[0])
            b1 = math.sqrt(x[2]) if x[2] > 0 else 0.0
        if x[1] < 0:
            b0 = -b0
        Betas.append([b0, b1, 0.0 if len(cols) == 3 else div(x[3], b0), 0.0])
    Rs, ts, errs = [], [], []
    for a in range(3):
        betas = Betas[a]
        gauss_newton(L, rho, betas)
        # compute_R_and_t (:543-553): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                for k in range(3):
                    ccs[j][k] += betas[i] * null[i][3 * j + k]
        pcs = [[al[0] * ccs[0][j] + al[1] * ccs[1][j] + al[2] * ccs[2][j] + al[3] * ccs[3][j] for j in range(3)] for al in alphas]
        if (pcs[0][2] < 0.0 and signs[0] > 0) or (pcs[0][2] > 0.0 and signs[0] < 0):
            pcs = [[-x for x in pc] for pc in pcs]
        pc0, pw0 = [0.0] * 3, [0.0] * 3
        for i in range(nc):
            for j in range(3):
                pc0[j] += pcs[i][j]
                pw0[j] += pws[i][j]
        for j in range(3):
            pc0[j] /= fnc
            pw0[j] /= fnc
        Abt = [[0.0] * 3 for _ in range(3)]
        for i in range(nc):
            for j in range(3):
                for k in range(3):
                    Abt[j][k] += (pcs[i][j] - pc0[j]) * (pws[i][k] - pw0[k])
        note("Abt", [list(r) for r in Abt])
        R, sweeps[5 + a] = linalg.rot(Abt)
        t = [pc0[i] - dot3(R[i], pw0) for i in range(3)]
        sum2 = 0.0
        for i in range(nc):
            pw = pws[i]
            Xc = dot3(R[0], pw) + t[0]
            Yc = dot3(R[1], pw) + t[1]
            inv_Zc = div(1.0, dot3(R[2], pw) + t[2])
            ue = 0.0 + 1.0 * Xc * inv_Zc
            ve = 0.0 + 1.0 * Yc * inv_Zc
            u, v = us[i]
            sum2 += sqrt_((u - ue) * (u - ue) + (v - ve) * (v - ve))
        Rs.append(R)
        ts.append(t)
        errs.append(sum2 / fnc)
    N = 0
    if errs[1] < errs[0]:
        N = 1
    if errs[2] < errs[N]:
        N = 2
    return dict(R=Rs[N], t=ts[N], err=errs[N], N=N + 1, sweeps=sweeps)


def div(a, b):
    """IEEE division: Python raises where C++ gives an infinity or a NaN"""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)


def sqrt_(x):
    """IEEE sqrt: NaN for a negative or NaN argument"""
    if x != x or x < 0.0:
        return float("nan")
    return math.sqrt(x)


def is_inlier(R, t, pos_w, bearing, thr):
    """the loop body of check_inliers (:162-177); thr is a float, compared as a double"""
    pc = [((R[r][0] * pos_w[0] + R[r][1] * pos_w[1]) + R[r][2] * pos_w[2]) + t[r] for r in range(3)]
    num = (pc[0] * bearing[0] + pc[1] * bearing[1]) + pc[2] * bearing[2]
    cos = div(num, sqrt_((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]))
    return thr < cos, cos


# ---- D14: the samples
MASK = (1 << 64) - 1


def mix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def draw(seed, p, it, n):
    """four distinct indices of [0, n), n >= 4: four steps of a Fisher-Yates shuffle of 0 .. n-1, step k swapping position k with position
    k + r_k mod (n - k), r_k the high 32 bits of mix64(base + (k + 1) * 0x9E3779B97F4A7C15)"""
    base = mix64((seed & MASK) ^ mix64((((p & 0xFFFFFFFF) << 32) | (it & 0xFFFFFFFF))))
    a = {}
    out = []
    for k in range(4):
        r = mix64((base + (k + 1) * 0x9E3779B97F4A7C15) & MASK)
        j = k + (r >> 32) % (n - k)
        aj, ak = a.get(j, j), a.get(k, k)
        out.append(aj)
        a[j], a[k] = ak, aj
    return out


OK, TOO_FEW_MATCHES, TOO_FEW_INLIERS = range(3)


def find_via_ransac(valid, bearing, pos_w, octave, scale_factors, iters=30, min_num_inliers=10, recompute=True, samples=None, seed=0, p=0, linalg=Jacobi,
                    trace=None):
    """constructor + find_via_ransac (:36-153) of one problem in slot form.  Returns dict(status, num_matches, R rows, t, num_inliers, best_iter,
    inliers per slot, hyp_inliers, cos_margin: the smallest |cos - thr| / thr over all inlier tests made)"""
    thr_tab = thresholds(scale_factors)
    slots = [s for s in range(len(valid)) if valid[s]]
    n = len(slots)
    B = [list(map(float, bearing[s])) for s in slots]
    W = [list(map(float, pos_w[s])) for s in slots]
    thr = [thr_tab[octave[s]] if 0 <= octave[s] < len(thr_tab) else None for s in slots]
    res = dict(status=OK, num_matches=n, R=[[0.0] * 3 for _ in range(3)], t=[0.0] * 3, num_inliers=0, best_iter=-1, inliers=[0] * len(valid),
               hyp_inliers=[0] * iters, cos_margin=INF)
    if n < 4 or n < min_num_inliers:
        res["status"] = TOO_FEW_MATCHES
        return res

    def flags_of(R, t):
        flags = []
        for k in range(n):
            if thr[k] is None:
                flags.append(0)
                continue
            inl, cos = is_inlier(R, t, W[k], B[k], thr[k])
            if cos == cos:
                res["cos_margin"] = min(res["cos_margin"], abs(cos - thr[k]) / thr[k])
            flags.append(1 if inl else 0)
        return flags

    best, best_flags, best_count, best_iter = None, [0] * n, 0, -1
    for it in range(iters):
        idx = list(samples[it]) if samples is not None else draw(seed, p, it, n)
        if any(not (0 <= i < n) for i in idx) or len(set(idx)) != 4:
            continue
        pose = compute_pose([W[i] for i in idx], [B[i] for i in idx], linalg, trace)
        if pose is None:
            continue
        flags = flags_of(pose["R"], pose["t"])
        num = sum(flags)
        res["hyp_inliers"][it] = num
        if best_count < num:
            best, best_flags, best_count, best_iter = pose, flags, num, it
    res["num_inliers"] = best_count
    if not (best_count > min_num_inliers):
        res["status"] = TOO_FEW_INLIERS
        return res
    res["best_iter"] = best_iter
    for k in range(n):
        res["inliers"][slots[k]] = best_flags[k]
    if recompute:
        pose = compute_pose([W[k] for k in range(n) if best_flags[k]], [B[k] for k in range(n) if best_flags[k]], linalg, trace)
        if pose is not None:
            best = pose
    res["R"], res["t"] = best["R"], best["t"]
    return res
