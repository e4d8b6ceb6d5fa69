"""Plain-Python restatement of DESIGN.md section 5, D22: optimize::graph_optimizer::optimize of the reference (optimize/graph_optimizer.cc:53-350)
with g2o's Sim3 (log included), its Sim3 edge with the central-difference Jacobians and its Levenberg-Marquardt, written from those sources and
from D22.  The edge rules work on objects, dicts and sets as the text does; the algebra is plain loops over Python floats (IEEE f64, one rounding
per operation, no fused multiply-add).  What D15 / D16 fix (the quaternion arithmetic, sin / cos, exp, Sim3(update)) is pose_optimizer_ref.py's and
transform_optimizer_ref.py's.  The host build of csrc/pose_graph.hpp is held to this bit for bit (tests/test_pose_graph_cpu.py)."""
import math
import struct

import numpy as np

import pose_optimizer_ref as D15
import transform_optimizer_ref as D16
from pose_optimizer_ref import DBL_MAX, END_ITERATIONS, END_RHO_ZERO, END_TRIES, MAX_TRIES, NAN, NUMERIC_DELTA, _div, _sqrt, f32

MIN_WEIGHT = 100
OK, NO_EDGES, ENVELOPE_TOO_LARGE, TOO_MANY_EDGES, BAD_LOOP_KF = range(5)
LOOP_CONNECTION, PARENT, LOOP, COVIS = 1, 2, 3, 4
LM_OK, LM_ERASED, LM_NO_VERTEX = range(3)
SENTINEL = dict(status=0xEE, num_edges=-77, edges=-55, sim3_cw=-7.25, corrected_wc=-7.25, pose=-7.25, info=-33, chi2=-7.25)


# ---- log and acos (fdlibm's e_log.c and e_acos.c, Horner, the domains of D22)
def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def log(x):
    if not (1e-300 <= x <= 1e300):
        return NAN
    b = _bits(x)
    hx = b >> 32
    k = (hx >> 20) - 1023
    hx &= 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    hx |= i ^ 0x3ff00000
    k += i >> 20
    m = _from_bits((hx << 32) | (b & 0xffffffff))
    f = m - 1.0
    s = f / (2.0 + f)
    dk = float(k)
    z = s * s
    R = z * (6.666666666666735130e-01 + z * (3.999999999940941908e-01 + z * (2.857142874366239149e-01 + z * (2.222219843214978396e-01 +
        z * (1.818357216161805012e-01 + z * (1.531383769920937332e-01 + z * 1.479819860511658591e-01))))))
    hfsq = (0.5 * f) * f
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f)


def _acos_r(z):
    p = z * (1.66666666666666657415e-01 + z * (-3.25565818622400915405e-01 + z * (2.01212532134862925881e-01 + z * (-4.00555345006794114027e-02 +
        z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))))
    q = 1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)))
    return p / q


def acos(x):
    pio2_hi, pio2_lo, pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
    if not (-1.0 <= x <= 1.0):
        return NAN
    if x == 1.0:
        return 0.0
    if x == -1.0:
        return pi + 2.0 * pio2_lo
    if abs(x) < 0.5:
        if abs(x) < 2.0 ** -57:
            return pio2_hi + pio2_lo
        return pio2_hi - (x - (pio2_lo - x * _acos_r(x * x)))
    if x < 0.0:
        z = (1.0 + x) * 0.5
        s = math.sqrt(z)
        w = _acos_r(z) * s - pio2_lo
        return pi - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = _from_bits(_bits(s) & 0xffffffff00000000)
    c = (z - df * df) / (s + df)
    w = _acos_r(z) * s + c
    return 2.0 * (df + w)


# ---- g2o's Sim3::log
def lu3_solve(W, t):
    """W x = t by LU with partial pivoting (the largest |a|, the first among equals), W row-major"""
    r = [[W[0], W[1], W[2], t[0]], [W[3], W[4], W[5], t[1]], [W[6], W[7], W[8], t[2]]]
    p = 0
    if abs(r[1][0]) > abs(r[p][0]):
        p = 1
    if abs(r[2][0]) > abs(r[p][0]):
        p = 2
    r[0], r[p] = r[p], r[0]
    l10, l20 = _div(r[1][0], r[0][0]), _div(r[2][0], r[0][0])
    for j in range(1, 4):
        r[1][j] = r[1][j] - l10 * r[0][j]
        r[2][j] = r[2][j] - l20 * r[0][j]
    if abs(r[2][1]) > abs(r[1][1]):
        r[1], r[2] = r[2], r[1]
    l21 = _div(r[2][1], r[1][1])
    r[2][2] = r[2][2] - l21 * r[1][2]
    r[2][3] = r[2][3] - l21 * r[1][3]
    x2 = _div(r[2][3], r[2][2])
    x1 = _div(r[1][3] - r[1][2] * x2, r[1][1])
    x0 = _div((r[0][3] - r[0][1] * x1) - r[0][2] * x2, r[0][0])
    return [x0, x1, x2]


def log_branch(est):
    """which of the four branches Sim3::log takes: (|sigma| < eps, d > 1 - eps)"""
    R = D15.rot_from_quat(est)
    return abs(log(est[7])) < 0.00001, 0.5 * (((R[0] + R[4]) + R[8]) - 1.0) > 1.0 - 0.00001


def sim3_log(est):
    s = est[7]
    sigma = log(s)
    R = D15.rot_from_quat(est)
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0)
    eps = 0.00001
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    if abs(sigma) < eps:
        C = 1.0
        if d > 1.0 - eps:
            k, A, B = 0.5, 0.5, 1.0 / 6.0
        else:
            theta = acos(d)
            th2 = theta * theta
            si, co = D15.sincos(theta)
            k = _div(theta, 2.0 * _sqrt(1.0 - d * d))
            A = _div(1.0 - co, th2)
            B = _div(theta - si, th2 * theta)
    else:
        C = _div(s - 1.0, sigma)
        sg2 = sigma * sigma
        if d > 1.0 - eps:
            k = 0.5
            A = _div((sigma - 1.0) * s + 1.0, sg2)
            B = _div(((0.5 * sg2 - sigma) + 1.0) * s, sg2 * sigma)
        else:
            theta = acos(d)
            th2 = theta * theta
            si, co = D15.sincos(theta)
            k = _div(theta, 2.0 * _sqrt(1.0 - d * d))
            sa, sb, cc = s * si, s * co, th2 + sg2
            A = _div(sa * sigma + (1.0 - sb) * theta, theta * cc)
            B = _div((C - _div((sb - 1.0) * sigma + sa * theta, cc)) * 1.0, th2)
    a, b, c = k * dR[0], k * dR[1], k * dR[2]
    O = [0.0, -c, b, c, 0.0, -a, -b, a, 0.0]
    O2 = [-(b * b + c * c), a * b, a * c, a * b, -(a * a + c * c), b * c, a * c, b * c, -(a * a + b * b)]
    W = [A * O[i] + B * O2[i] for i in range(9)]
    for i in (0, 4, 8):
        W[i] = W[i] + C
    return [a, b, c] + lu3_solve(W, est[4:7]) + [sigma]


def edge_error(C, v1, v2):
    return sim3_log(D16.mul(D16.mul(C, v1), D16.inverse(v2)))


def sim3_from_pose(pose):
    return D15.quat_from_rot([float(v) for v in pose[:9]]) + [float(pose[9]), float(pose[10]), float(pose[11]), 1.0]


def pose_from_sim3(est):
    s = float(f32(est[7]))
    R = D15.rot_from_quat(est)
    t = [_div(est[4], s), _div(est[5], s), _div(est[6], s)]
    return R + t + [((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2] for i in range(3)]


# ---- the map as the text sees it
class Keyframe:
    def __init__(self, row, tables):
        F = len(tables["kf_parent"])
        self.row, self.id_ = row, int(tables["kf_id"][row]) if tables.get("kf_id") is not None else row
        self.erased = bool(tables["kf_erased"][row]) if tables.get("kf_erased") is not None else False
        self.pose = [float(v) for v in tables["pose"][row]]
        p = int(tables["kf_parent"][row])
        self.parent = p if 0 <= p < F else None
        n = min(max(int(tables["kf_n_conn"][row]), 0), tables["kf_conn"].shape[1])
        self.connected = {}
        for c, w in zip(tables["kf_conn"][row, :n].tolist(), tables["kf_conn_w"][row, :n].tolist()):
            self.connected.setdefault(c, w)
        n = min(max(int(tables["kf_n_covis"][row]), 0), tables["kf_covis"].shape[1])
        self.ordered, self.ordered_w = tables["kf_covis"][row, :n].tolist(), tables["kf_covis_w"][row, :n].tolist()
        if tables.get("kf_loop_offsets") is not None:
            lo, hi = int(tables["kf_loop_offsets"][row]), int(tables["kf_loop_offsets"][row + 1])
            self.loop_edges = tables["kf_loop"][lo:max(hi, lo)].tolist()
        else:
            self.loop_edges = []

    def get_weight(self, c):
        return self.connected.get(c, 0)

    def get_covisibilities_over_weight(self, weight, events):
        if not self.ordered:
            return []
        itr = next((i for i, v in enumerate(self.ordered_w) if not v >= weight), len(self.ordered_w))
        if itr == len(self.ordered_w):
            events.add("over_weight_all_qualify_returns_empty")
            return []
        if itr > 0:
            events.add("over_weight_proper_prefix")
        return self.ordered[:itr]


def build(tables, pr, events=None):
    """[2] and [3]: (status, keyframes, Sim3s_cw {row: Sim3}, edges [(id1 row, id2 row, type, Sim3_21)]).  pr: dict(loop_kf, curr_kf, pre_corrected,
    non_corrected, loop_connections)"""
    ev = events if events is not None else set()
    F = len(tables["kf_parent"])
    kfs = [Keyframe(r, tables) for r in range(F)]
    is_vertex = lambda r: 0 <= r < F and not kfs[r].erased
    loop_kf, curr_kf = int(pr["loop_kf"]), int(pr["curr_kf"])
    if not is_vertex(loop_kf):
        return BAD_LOOP_KF, kfs, {}, []
    pre, non = pr.get("pre_corrected") or {}, pr.get("non_corrected") or {}
    Sim3s_cw = {}
    for kf in kfs:
        if kf.erased:
            ev.add("erased_keyframe_is_no_vertex")
            continue
        if kf.row in pre:
            ev.add("pre_corrected_vertex")
            Sim3s_cw[kf.row] = [float(v) for v in pre[kf.row]]
        else:
            Sim3s_cw[kf.row] = sim3_from_pose(kf.pose)
    edges, inserted_edge_pairs = [], set()

    def insert_edge(a, b, kind, Sim3_21):
        if a == b or not is_vertex(a) or not is_vertex(b):
            ev.add("edge_with_a_missing_end_not_inserted")
            return
        edges.append((a, b, kind, Sim3_21))
        inserted_edge_pairs.add((min(kfs[a].id_, kfs[b].id_), max(kfs[a].id_, kfs[b].id_)))
        ev.add(("edge", kind))

    # [3.1]
    for a in sorted((pr.get("loop_connections") or {}).keys()):
        for b in sorted(pr["loop_connections"][a]):
            if not is_vertex(a) or not is_vertex(b) or a == b:
                ev.add("edge_with_a_missing_end_not_inserted")
                continue
            exempt = is_vertex(curr_kf) and kfs[a].id_ == kfs[curr_kf].id_ and kfs[b].id_ == kfs[loop_kf].id_
            if not exempt and kfs[a].get_weight(b) < MIN_WEIGHT:
                ev.add("loop_connection_below_weight_skipped")
                continue
            if exempt and kfs[a].get_weight(b) < MIN_WEIGHT:
                ev.add("curr_loop_exempt_from_weight")
            insert_edge(a, b, LOOP_CONNECTION, D16.mul(Sim3s_cw[b], D16.inverse(Sim3s_cw[a])))
    # [3.2]
    def sim3_of(r):
        if r in non:
            ev.add("non_corrected_used")
            return [float(v) for v in non[r]]
        return Sim3s_cw[r]

    for kf in kfs:
        if kf.erased:
            continue
        id1 = kf.id_
        Sim3_w1 = D16.inverse(sim3_of(kf.row))
        parent = kf.parent
        if parent is not None:
            if id1 <= kfs[parent].id_:
                ev.add("parent_id_not_below_leaves_the_keyframe")
                continue
            if is_vertex(parent):
                insert_edge(kf.row, parent, PARENT, D16.mul(sim3_of(parent), Sim3_w1))
            else:
                ev.add("edge_with_a_missing_end_not_inserted")
        for c in kf.loop_edges:
            if not is_vertex(c):
                ev.add("edge_with_a_missing_end_not_inserted")
                continue
            if id1 <= kfs[c].id_:
                ev.add("loop_edge_id_skip")
                continue
            insert_edge(kf.row, c, LOOP, D16.mul(sim3_of(c), Sim3_w1))
        for c in kf.get_covisibilities_over_weight(MIN_WEIGHT, ev):
            if not 0 <= c < F or parent is None:
                ev.add("covis_without_parent")
                continue
            if kfs[c].id_ == kfs[parent].id_:
                ev.add("covis_is_the_parent")
                continue
            if kfs[c].parent == kf.row:
                ev.add("covis_is_a_child")
                continue
            if c in set(kf.loop_edges):
                ev.add("covis_is_a_loop_edge")
                continue
            if kfs[c].erased:
                ev.add("covis_is_erased")
                continue
            if id1 <= kfs[c].id_:
                ev.add("covis_id_skip")
                continue
            if (min(id1, kfs[c].id_), max(id1, kfs[c].id_)) in inserted_edge_pairs:
                ev.add("covis_pair_already_inserted")
                continue
            insert_edge(kf.row, c, COVIS, D16.mul(sim3_of(c), Sim3_w1))
    return (OK if edges else NO_EDGES), kfs, Sim3s_cw, edges


class Graph:
    """the optimisation of one problem"""

    def __init__(self, tables, pr, edge_cap=1 << 14, env_cap=1 << 16, events=None):
        self.ev = events if events is not None else set()
        self.pr, self.fix_scale = pr, bool(pr.get("fix_scale"))
        self.status, self.kfs, self.Sim3s_cw, self.edges = build(tables, pr, self.ev)
        self.num_edges = len(self.edges)
        self.est = dict(self.Sim3s_cw)
        self.info, self.chi2, self.lam = [0, 0, 0, 0], 0.0, 0.0
        if self.status == OK and self.num_edges > edge_cap:
            self.status, self.edges = TOO_MANY_EDGES, []
        if self.status != OK:
            return
        touched = {a for a, b, _, _ in self.edges} | {b for a, b, _, _ in self.edges}
        if len(touched) < len(self.Sim3s_cw):
            self.ev.add("vertex_without_edges")
        self.sys = [r for r in sorted(touched) if r != int(pr["loop_kf"])]
        self.idx = {r: i for i, r in enumerate(self.sys)}
        n = len(self.sys)
        self.first = list(range(n))
        self.inc = [[] for _ in range(n)]
        for e, (a, b, _, _) in enumerate(self.edges):
            ia, ib = self.idx.get(a, -1), self.idx.get(b, -1)
            for i, o in ((ia, ib), (ib, ia)):
                if i >= 0:
                    self.inc[i].append(e)
                    if 0 <= o < self.first[i]:
                        self.first[i] = o
        if sum(i - f + 1 for i, f in enumerate(self.first)) > env_cap:
            self.status = ENVELOPE_TOO_LARGE
            return
        self.info[3] = n
        # components: is every vertex of the system connected to the fixed one?
        seen, todo = {int(pr["loop_kf"])}, [int(pr["loop_kf"])]
        while todo:
            r = todo.pop()
            for a, b, _, _ in self.edges:
                for u, v in ((a, b), (b, a)):
                    if u == r and v not in seen:
                        seen.add(v); todo.append(v)
        if any(r not in seen for r in self.sys):
            self.ev.add("component_without_the_fixed_vertex")

    # the error of every edge at est: (errors, chi2 per edge)
    def errors(self, est):
        out = []
        for a, b, _, C in self.edges:
            err = edge_error(C, est[a], est[b])
            chi = 0.0
            for m in range(7):
                chi = chi + err[m] * err[m]
            out.append((err, chi))
        return out

    def linearize(self):
        """H (dict (p, c) -> value on the lower skyline), b, the errors"""
        scalar = 1.0 / (2.0 * NUMERIC_DELTA)
        errs = self.errors(self.est)
        J = []
        for (a, b, _, C) in self.edges:
            blocks = []
            for end, r in enumerate((a, b)):
                if r not in self.idx:
                    blocks.append(None)
                    continue
                cols = []
                for d in range(7):
                    pm = []
                    for v in (NUMERIC_DELTA, -NUMERIC_DELTA):
                        u = [0.0] * 7
                        u[d] = v
                        moved = D16.oplus(u, self.est[r], self.fix_scale)
                        pm.append(edge_error(C, moved if end == 0 else self.est[a], moved if end == 1 else self.est[b]))
                    cols.append([scalar * (pm[0][m] - pm[1][m]) for m in range(7)])
                blocks.append(cols)                          # cols[d][m]
            J.append(blocks)
        n = len(self.sys)
        H, bvec = {}, [0.0] * (7 * n)
        for i in range(n):
            for k in range(self.first[i], i + 1):
                for r in range(7):
                    for c in range(7):
                        if k == i and c > r:
                            continue
                        acc = 0.0
                        for e in self.inc[i]:
                            a, b = self.edges[e][0], self.edges[e][1]
                            end = 0 if self.idx.get(a, -1) == i else 1
                            own = J[e][end]
                            if k == i:
                                oth = own
                            else:
                                if self.idx.get(b if end == 0 else a, -1) != k:
                                    continue
                                oth = J[e][1 - end]
                            term = own[r][0] * oth[c][0]
                            for m in range(1, 7):
                                term = term + own[r][m] * oth[c][m]
                            acc = acc + term
                        H[(7 * i + r, 7 * k + c)] = acc
            for r in range(7):
                acc = 0.0
                for e in self.inc[i]:
                    end = 0 if self.idx.get(self.edges[e][0], -1) == i else 1
                    own, err = J[e][end], errs[e][0]
                    term = own[r][0] * (-err[0])
                    for m in range(1, 7):
                        term = term + own[r][m] * (-err[m])
                    acc = acc + term
                bvec[7 * i + r] = acc
        return H, bvec, errs

    def optimize(self, max_iter=50):
        if self.status != OK:
            return
        n = len(self.sys)
        current, iterations, rejected, end, lam, ni = 0.0, 0, 0, 0, 0.0, 2.0
        for it in range(max_iter):
            H, b, errs = self.linearize()
            current = 0.0
            for _, chi in errs:
                current = current + chi
            if it == 0:
                self.start_chi = current
                m = 0.0
                for p in range(7 * n):
                    d = abs(H[(p, p)])
                    m = d if d > m else m
                lam, ni = 1e-5 * m, 2.0
            qmax, rho = 0, 0.0
            while True:
                x, ok = skyline_solve(H, self.first, b, lam)
                tried = dict(self.est)
                for i, r in enumerate(self.sys):
                    tried[r] = D16.oplus(x[7 * i:7 * i + 7], self.est[r], self.fix_scale)
                temp = 0.0
                for _, chi in self.errors(tried):
                    temp = temp + chi
                temp_chi = temp if ok else DBL_MAX
                scale = 0.0
                for i in range(n):
                    part = 0.0
                    for k in range(7):
                        part = part + x[7 * i + k] * (lam * x[7 * i + k] + b[7 * i + k])
                    scale = scale + part
                scale = scale + 1e-3
                rho = _div(current - temp_chi, scale)
                if rho > 0.0 and -DBL_MAX <= temp_chi <= DBL_MAX:
                    v = 2.0 * rho - 1.0
                    alpha = 1.0 - (v * v) * v
                    alpha = alpha if alpha < 2.0 / 3.0 else 2.0 / 3.0
                    lam = lam * (alpha if alpha > 1.0 / 3.0 else 1.0 / 3.0)
                    ni = 2.0
                    current = temp_chi
                    self.est = tried
                else:
                    lam = lam * ni
                    ni = ni * 2.0
                    rejected += 1
                qmax += 1
                if not (rho < 0.0 and qmax < MAX_TRIES):
                    break
            iterations += 1
            end = END_TRIES if qmax == MAX_TRIES else END_RHO_ZERO if rho == 0.0 else 0
            if end:
                break
        self.info = [iterations, rejected, end if end else (END_ITERATIONS if iterations else 0), n]
        self.chi2, self.lam = current, lam


def skyline_solve(H, first, b, lam):
    """(H + lam I) x = b by the Cholesky of the block skyline in vertex order; H: {(p, c): value} on the lower skyline.  Returns (x, ok)."""
    N = 7 * len(first)
    fc = [7 * first[p // 7] for p in range(N)]
    L = {}
    dl = [0.0] * N
    for j in range(N):
        s = H[(j, j)] + lam
        for k in range(fc[j], j):
            s = s - L[(j, k)] * L[(j, k)]
        if not (s > 0.0) or s > DBL_MAX:
            return [0.0] * N, False
        d = math.sqrt(s)
        dl[j] = d
        for p in range(j + 1, N):
            if fc[p] > j:
                continue
            v = H[(p, j)]
            for k in range(max(fc[j], fc[p]), j):
                v = v - L[(p, k)] * L[(j, k)]
            L[(p, j)] = _div(v, d)
    v = list(b)
    y = [0.0] * N
    for j in range(N):
        y[j] = _div(v[j], dl[j])
        for p in range(j + 1, N):
            if fc[p] <= j:
                v[p] = v[p] - L[(p, j)] * y[j]
    v = list(y)
    x = [0.0] * N
    for j in range(N - 1, -1, -1):
        x[j] = _div(v[j], dl[j])
        for p in range(fc[j], j):
            v[p] = v[p] - L[(j, p)] * x[j]
    return x, True


def run(tables, problems, edge_cap=1 << 14, env_cap=1 << 16, max_iter=50, events=None, solve=True):
    out = []
    for pr in problems:
        g = Graph(tables, pr, edge_cap, env_cap, events)
        if solve:
            g.optimize(max_iter)
        out.append(g)
    return out


def expected(graphs, F, edge_cap, names=None):
    """sentinel-filled arrays as the library leaves them"""
    G = len(graphs)
    shapes = dict(status=((G,), np.uint8), num_edges=((G,), np.int32), edges=((G, edge_cap, 3), np.int32), sim3_cw=((G, F, 8), np.float64),
                  corrected_wc=((G, F, 8), np.float64), pose=((G, F, 15), np.float64), info=((G, 4), np.int32), chi2=((G, 2), np.float64))
    o = {k: np.full(s, SENTINEL[k], dt) for k, (s, dt) in shapes.items() if names is None or k in names}
    for g, gr in enumerate(graphs):
        o["status"][g] = gr.status
        if "num_edges" in o:
            o["num_edges"][g] = gr.num_edges
        if gr.status not in (OK, NO_EDGES):
            continue
        if "edges" in o:
            for e, (a, b, kind, _) in enumerate(gr.edges):
                o["edges"][g, e] = (a, b, kind)
        for r, s in gr.Sim3s_cw.items():
            if "sim3_cw" in o:
                o["sim3_cw"][g, r] = s
            if "corrected_wc" in o:
                o["corrected_wc"][g, r] = D16.inverse(gr.est[r])
            if "pose" in o:
                o["pose"][g, r] = pose_from_sim3(gr.est[r])
        if "info" in o:
            o["info"][g] = gr.info
        if "chi2" in o:
            o["chi2"][g] = (gr.chi2, gr.lam)
    return o


def correct_landmarks(pos_w, ref_kf, sim3_cw, corrected_wc, lm_erased, kf_erased, sentinel=-7.25):
    L, F = len(pos_w), len(sim3_cw)
    out, status = np.full((L, 3), sentinel), np.zeros(L, np.uint8)
    for l in range(L):
        if lm_erased is not None and lm_erased[l]:
            status[l] = LM_ERASED
            continue
        r = int(ref_kf[l])
        if not 0 <= r < F or (kf_erased is not None and kf_erased[r]):
            status[l] = LM_NO_VERTEX
            continue
        p = D16.sim3_map([float(v) for v in sim3_cw[r]], [float(v) for v in pos_w[l]])
        out[l] = D16.sim3_map([float(v) for v in corrected_wc[r]], p)
    return out, status
