"""solve::sim3_solver (src/PLPSLAM/solve/sim3_solver.cc) restated in plain Python: Python floats for the reference's doubles, numpy.float32
where it holds floats, every sum left to right, the reference's RANSAC loop literally (sequential, `max_num_inliers < num_inliers`).  The
eigenvector of Horn's matrix is the Jacobi of DESIGN.md section 5, D13, written out; `eig=` swaps another one in (numpy.linalg.eigh).  asin /
atan2 of the equirectangular camera are math's (glibc).  Written from the reference's sources and D13, not from csrc/sim3.hpp."""
import math

import numpy as np

F32 = np.float32
SWEEP_LIMIT = 30
SKIP_TOL = 2.0 ** -106
CHI_SQ_2D = F32(9.21034)                      # sim3_solver.cc:67
OK, TOO_FEW_POINTS, TOO_FEW_INLIERS = 0, 1, 2
PERSPECTIVE, FISHEYE, EQUIRECTANGULAR = 0, 1, 2
MASK64 = (1 << 64) - 1


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- D13: the unit eigenvector of the largest eigenvalue of a symmetric 4 x 4 matrix
def sym_eig4_max(N):
    """N: 4 x 4 nested lists / array, the upper triangle is read.  Returns (v list of 4, sweeps, eigenvalues list of 4)."""
    S = [[float(N[min(i, j)][max(i, j)]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    n = 0
    while n < SWEEP_LIMIT:
        rotated = False
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            apq, app, aqq = S[p][q], S[p][p], S[q][q]
            if not (apq * apq > SKIP_TOL * (app * app + aqq * aqq)):
                continue
            theta = (aqq - app) / (2.0 * apq)
            root = math.sqrt(1.0 + theta * theta)
            t = 1.0 / (theta + root) if theta >= 0.0 else -1.0 / (root - theta)
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            for k in range(4):
                if k == p or k == q:
                    continue
                akp, akq = S[k][p], S[k][q]
                S[k][p] = S[p][k] = c * akp - s * akq
                S[k][q] = S[q][k] = s * akp + c * akq
            S[p][p] = app - t * apq
            S[q][q] = aqq + t * apq
            S[p][q] = S[q][p] = 0.0
            for r in range(4):
                vp, vq = V[r][p], V[r][q]
                V[r][p] = c * vp - s * vq
                V[r][q] = s * vp + c * vq
            rotated = True
        if not rotated:
            break
        n += 1
    best, lb = 0, S[0][0]
    for i in (1, 2, 3):
        if S[i][i] > lb:
            best, lb = i, S[i][i]
    return [V[r][best] for r in range(4)], n, [S[i][i] for i in range(4)]


def eig_jacobi(N):
    return sym_eig4_max(N)[0]


def eig_eigh(N):
    """numpy.linalg.eigh in place of the Jacobi: the eigenvector of the largest eigenvalue"""
    w, V = np.linalg.eigh(np.asarray(N, np.float64))
    return [float(x) for x in V[:, 3]]


def horn_matrix(pts_1, pts_2):
    """N of sim3_solver.cc:226-229 (with the centred points and centroids): pts row-major 3 x 3 nested lists, column c = sample c"""
    c1 = [((pts_1[r][0] + pts_1[r][1]) + pts_1[r][2]) / 3.0 for r in range(3)]
    c2 = [((pts_2[r][0] + pts_2[r][1]) + pts_2[r][2]) / 3.0 for r in range(3)]
    a1 = [[pts_1[r][c] - c1[r] for c in range(3)] for r in range(3)]
    a2 = [[pts_2[r][c] - c2[r] for c in range(3)] for r in range(3)]
    M = [[(a1[i][0] * a2[j][0] + a1[i][1] * a2[j][1]) + a1[i][2] * a2[j][2] for j in range(3)] for i in range(3)]
    Sxx, Syx, Szx, Sxy, Syy, Szy, Sxz, Syz, Szz = M[0][0], M[1][0], M[2][0], M[0][1], M[1][1], M[2][1], M[0][2], M[1][2], M[2][2]
    N = [[(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
         [Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz],
         [Szx - Sxz, Sxy + Syx, (-Sxx + Syy) - Szz, Syz + Szy],
         [Sxy - Syx, Szx + Sxz, Syz + Szy, (-Sxx - Syy) + Szz]]
    return N, c1, c2, a1, a2


def horn_sim3(pts_1, pts_2, fix_scale, eig=eig_jacobi):
    """sim3_solver::compute_Sim3 (:193-288).  Returns dict(rot_12, trans_12, scale_12, rot_21, trans_21, scale_21): nested lists, floats, F32 scales"""
    N, c1, c2, a1, a2 = horn_matrix(pts_1, pts_2)
    e = list(eig(N))
    e2 = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]
    if e2 > 0.0:
        en = math.sqrt(e2)
        e = [x / en for x in e]
    qn = math.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3])
    w, x, y, z = [_div(v, qn) for v in e]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]
    if fix_scale:
        s21 = F32(1.0)
    else:
        denom = numer = 0.0
        for c in range(3):
            for r in range(3):
                in2 = (R[r][0] * a1[0][c] + R[r][1] * a1[1][c]) + R[r][2] * a1[2][c]
                denom = denom + a1[r][c] * a1[r][c]
                numer = numer + a2[r][c] * in2
        with np.errstate(all="ignore"):
            s21 = F32(_div(numer, denom))
    s = float(s21)
    t21 = [c2[r] - (((s * R[r][0]) * c1[0] + (s * R[r][1]) * c1[1]) + (s * R[r][2]) * c1[2]) for r in range(3)]
    R12 = [[R[c][r] for c in range(3)] for r in range(3)]
    with np.errstate(all="ignore"):
        s12 = F32(_div(1.0, float(s21)))
    ns = float(-s12)
    t12 = [((ns * R12[r][0]) * t21[0] + (ns * R12[r][1]) * t21[1]) + (ns * R12[r][2]) * t21[2] for r in range(3)]
    return dict(rot_12=R12, trans_12=t12, scale_12=s12, rot_21=R, trans_21=t21, scale_21=s21)


# ---- camera::*::reproject_to_image (perspective.cc:190-209, fisheye.cc:231-249, equirectangular.cc:104-119): (u, v) or None = not written
def reproject(cam, rot, trans, x):
    xc = ((rot[0][0] * x[0] + rot[0][1] * x[1]) + rot[0][2] * x[2]) + trans[0]
    yc = ((rot[1][0] * x[0] + rot[1][1] * x[1]) + rot[1][2] * x[2]) + trans[1]
    zc = ((rot[2][0] * x[0] + rot[2][1] * x[1]) + rot[2][2] * x[2]) + trans[2]
    if cam["model"] == EQUIRECTANGULAR:
        sq = (xc * xc + yc * yc) + zc * zc
        bx, by, bz = xc, yc, zc
        if sq > 0.0:
            s = math.sqrt(sq)
            bx, by, bz = xc / s, yc / s, zc / s
        lat = -(math.asin(by) if -1.0 <= by <= 1.0 else math.nan)
        lon = math.atan2(bx, bz)
        return (cam["cols"] * (0.5 + lon / (2.0 * 3.14159265358979323846)), cam["rows"] * (0.5 - lat / 3.14159265358979323846))
    if not (zc > 0.0):      # `if (pos_c(2) <= 0.0) return false` -- a NaN depth is written by the reference and is no inlier either way
        if zc != zc:
            return (math.nan, math.nan)
        return None
    z_inv = 1.0 / zc
    return ((cam["fx"] * xc) * z_inv + cam["cx"], (cam["fy"] * yc) * z_inv + cam["cy"])


IDENTITY = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def draw(seed, p, it, n):
    """D13's generator: three distinct indices of [0, n) by a partial Fisher-Yates shuffle driven by splitmix64's finaliser"""
    def mix(x):
        x &= MASK64
        x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & MASK64
        x ^= x >> 27; x = (x * 0x94D049BB133111EB) & MASK64
        x ^= x >> 31
        return x
    base = mix((seed & MASK64) ^ mix(((p & 0xFFFFFFFF) << 32) | (it & 0xFFFFFFFF)))
    a = list(range(n))
    out = []
    for k in range(3):
        r = mix(base + (k + 1) * 0x9E3779B97F4A7C15)
        j = k + (r >> 32) % (n - k)
        a[k], a[j] = a[j], a[k]
        out.append(a[k])
    return out


class Sim3Solver:
    """the reference's class over the flattened lists of one problem (include/plp_front.h: plp_sim3_ransac_args)"""

    def __init__(self, cam, valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, sigma_sq_1, sigma_sq_2, fix_scale, min_num_inliers, eig=eig_jacobi):
        self.cam, self.fix_scale, self.min_num_inliers, self.eig = cam, bool(fix_scale), int(min_num_inliers), eig
        self.slots, self.x1, self.x2, self.thr1, self.thr2, self.never = [], [], [], [], [], []
        P1, P2 = [float(v) for v in pose_1], [float(v) for v in pose_2]
        cam_pt = lambda P, w: [((P[3 * r] * w[0] + P[3 * r + 1] * w[1]) + P[3 * r + 2] * w[2]) + P[9 + r] for r in range(3)]
        for i in range(len(valid)):                      # :70-115
            if not valid[i]:
                continue
            self.slots.append(i)
            self.x1.append(cam_pt(P1, [float(v) for v in pos_w_1[i]]))
            self.x2.append(cam_pt(P2, [float(v) for v in pos_w_2[i]]))
            o1, o2 = int(octave_1[i]), int(octave_2[i])
            lv = 0 <= o1 < len(sigma_sq_1) and 0 <= o2 < len(sigma_sq_2)
            self.thr1.append(CHI_SQ_2D * F32(sigma_sq_1[o1]) if lv else F32(0))
            self.thr2.append(CHI_SQ_2D * F32(sigma_sq_2[o2]) if lv else F32(0))
            self.never.append(not lv)
        self.n = len(self.slots)
        zero = [0.0, 0.0, 0.0]
        self.rep1 = [reproject(cam, IDENTITY, zero, x) for x in self.x1]     # :117-118
        self.rep2 = [reproject(cam, IDENTITY, zero, x) for x in self.x2]
        for k in range(self.n):                          # D13: behind its own camera -> never an inlier
            if self.rep1[k] is None or self.rep2[k] is None:
                self.never[k] = True

    def hypothesis(self, idx):
        pts_1 = [[self.x1[idx[c]][r] for c in range(3)] for r in range(3)]
        pts_2 = [[self.x2[idx[c]][r] for c in range(3)] for r in range(3)]
        return horn_sim3(pts_1, pts_2, self.fix_scale, self.eig)

    def count_inliers(self, H, margins=None):
        """:290-325; margins: a list that receives |error - threshold| / threshold of every comparison made"""
        s21, s12 = float(H["scale_21"]), float(H["scale_12"])
        m21 = [[s21 * v for v in row] for row in H["rot_21"]]
        m12 = [[s12 * v for v in row] for row in H["rot_12"]]
        flags = []
        for k in range(self.n):
            a = reproject(self.cam, m21, H["trans_21"], self.x1[k])
            b = reproject(self.cam, m12, H["trans_12"], self.x2[k])
            if self.never[k] or a is None or b is None:
                flags.append(0)
                continue
            d2 = (a[0] - self.rep2[k][0], a[1] - self.rep2[k][1])
            d1 = (b[0] - self.rep1[k][0], b[1] - self.rep1[k][1])
            e2 = d2[0] * d2[0] + d2[1] * d2[1]
            e1 = d1[0] * d1[0] + d1[1] * d1[1]
            t2, t1 = float(self.thr2[k]), float(self.thr1[k])
            if margins is not None:
                for e, t in ((e2, t2), (e1, t1)):
                    if t > 0.0 and e == e:
                        margins.append(abs(e - t) / t)
            flags.append(1 if (e2 < t2 and e1 < t1) else 0)
        return flags

    def find_via_ransac(self, samples, hook=None):
        """samples: a list of index triples, one per iteration.  Returns dict(status, num_common, rot_12, trans_12, scale_12, num_inliers, best_iter,
        inliers (per slot), hyp_inliers).  hook(iter, H, flags) is called for every hypothesis that was formed."""
        iters = len(samples)
        res = dict(num_common=self.n, rot_12=[[0.0] * 3 for _ in range(3)], trans_12=[0.0] * 3, scale_12=F32(0), num_inliers=0, best_iter=-1,
                   hyp_inliers=[0] * iters, inlier_ranks=[0] * self.n)
        if self.n < 3 or self.n < self.min_num_inliers:          # :130
            res["status"] = TOO_FEW_POINTS
            return res
        max_num_inliers, best, best_flags, best_iter = 0, None, None, -1
        for it in range(iters):                                   # :145
            idx = [int(v) for v in samples[it]]
            if not all(0 <= v < self.n for v in idx) or len(set(idx)) != 3:
                continue                                          # the library's rule for a caller's bad sample: 0 inliers
            H = self.hypothesis(idx)
            flags = self.count_inliers(H)
            num = sum(flags)
            res["hyp_inliers"][it] = num
            if hook:
                hook(it, H, flags)
            if max_num_inliers < num:                             # :168
                max_num_inliers, best, best_flags, best_iter = num, H, flags, it
        res["num_inliers"] = max_num_inliers
        if max_num_inliers < self.min_num_inliers:                # :177
            res["status"] = TOO_FEW_INLIERS
            return res
        res["status"] = OK
        if best is not None:
            res.update(rot_12=best["rot_12"], trans_12=best["trans_12"], scale_12=best["scale_12"], best_iter=best_iter, inlier_ranks=best_flags)
        return res


def run_problem(cam, prob, samples, fix_scale, min_num_inliers, eig=eig_jacobi, seed=None, p=0, hook=None):
    """one problem of a scene (sim3_solver_scene.problem's dict) -> the outputs as numpy arrays shaped like the library's, inliers in slot order"""
    count = int(prob.get("count", len(prob["valid"])))
    s = Sim3Solver(cam, prob["valid"][:count], prob["pos_w_1"], prob["pos_w_2"], prob["octave_1"], prob["octave_2"], prob["pose_1"], prob["pose_2"],
                   prob["sigma_sq_1"], prob["sigma_sq_2"], fix_scale, min_num_inliers, eig)
    if samples is None:
        iters = prob["iters"]
        samples = [draw(seed, p, it, s.n) for it in range(iters)] if s.n >= 3 else [[0, 0, 0]] * iters
    r = s.find_via_ransac(samples, hook)
    inl = np.zeros(len(prob["valid"]), np.uint8)
    for k, f in enumerate(r["inlier_ranks"]):
        inl[s.slots[k]] = f
    return dict(status=np.uint8(r["status"]), num_common=np.int32(r["num_common"]), rot_12=np.array(r["rot_12"], np.float64),
                trans_12=np.array(r["trans_12"], np.float64), scale_12=F32(r["scale_12"]), num_inliers=np.int32(r["num_inliers"]),
                best_iter=np.int32(r["best_iter"]), inliers=inl, hyp_inliers=np.array(r["hyp_inliers"], np.int32)), s
