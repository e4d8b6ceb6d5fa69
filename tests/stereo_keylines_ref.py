"""CPU restatement of the stereo key-line association (plp_stereo_keylines_*) and of the 3-D key lines (plp_keylines_3d_*):
the filter of the stereo data::frame constructors on BinaryDescriptorMatcher::match's result (data/frame.cc:389-427, again at :494-533) and
frame::triangulate_stereo_for_line (data/frame.cc:953-1123), written from the reference's sources with the numeric contract of DESIGN.md
section 5, D7: float32 where the reference computes in float, float64 scalars in the reference's order otherwise, every Eigen expression
written out left to right with all of its terms.  Key lines are records of plp.KL_DTYPE; a pose is the 15-double row of frame_pose."""
import numpy as np

from landmark_observe_ref import frame_pose  # noqa: F401  (re-exported for the tests)

f32, f64 = np.float32, np.float64
STEREO, RGBD = 1, 2


# ---------------------------------------------------------------------------------------------------------------- association
def point_distance(dx, dy):
    """sqrt(p.dot(p)) of a cv::Point2f difference: float dot x*x + y*y, square root rounded to float"""
    dx, dy = f32(dx), f32(dy)
    return f32(np.sqrt(f64(f32(f32(dx * dx) + f32(dy * dy)))))


def angle_deg(a1, a2, reading="float"):
    """abs((abs(a1) - abs(a2))) * 180 / 3.14 assigned to a float.  reading "float": std::abs(float) (what GCC's libstdc++ gives the
    unqualified call, D7); "int": C's abs(int), the float angles truncated to int"""
    if reading == "int":
        i1, i2 = int(f32(a1)), int(f32(a2))                 # float -> int conversion truncates toward zero
        return f32(f64(abs(abs(i1) - abs(i2)) * 180) / 3.14)
    d = f32(abs(f32(abs(f32(a1))) - f32(abs(f32(a2)))))
    return f32(f64(f32(d * f32(180.0))) / 3.14)


def keep_match(kl1, kl2, dist, reading="float"):
    """the three gates of frame.cc:400-418 for query line kl1, train line kl2 and DMatch.distance dist"""
    if not (f32(dist) < f32(30)):
        return False
    ds = point_distance(f32(kl1["startPointX"]) - f32(kl2["startPointX"]), f32(kl1["startPointY"]) - f32(kl2["startPointY"]))
    de = point_distance(f32(kl1["endPointX"]) - f32(kl2["endPointX"]), f32(kl1["endPointY"]) - f32(kl2["endPointY"]))
    ang = angle_deg(kl1["angle"], kl2["angle"], reading)
    return bool(ds < f32(200) and de < f32(200) and ang < f32(5))


def stereo_keylines(kl_left, kl_right, train_idx, dist, reading="float"):
    """one frame -> (good_match [n] i32, kl_depths [n, 2] f32, kl_x_right [n, 2] f32); -1 / (-1, -1) where no match is kept"""
    n, nr = len(kl_left), len(kl_right)
    good = np.full(n, -1, np.int32)
    for j in range(n):
        t = int(train_idx[j])
        if nr == 0 or not (0 <= t < nr):
            continue
        if keep_match(kl_left[j], kl_right[t], dist[j], reading):
            good[j] = t
    v = np.where(good >= 0, f32(1.0), f32(-1.0)).astype(np.float32)
    pair = np.stack([v, v], 1)
    return good, pair, pair.copy()


# ---------------------------------------------------------------------------------------------------------------- 3-D lines
class _Finite:
    """collects every intermediate: D7's "a non-finite intermediate gives the zero vector" checked on all of them"""

    def __init__(self):
        self.ok = True

    def __call__(self, *vals):
        for v in vals:
            if not np.all(np.isfinite(v)):
                self.ok = False
        return vals[0] if len(vals) == 1 else vals


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _plane(P, l):
    """line^T * P (equally P^T * line): plane(j) = (l0 P(0,j) + l1 P(1,j)) + l2 P(2,j)"""
    return [(l[0] * P[0][j] + l[1] * P[1][j]) + l[2] * P[2][j] for j in range(4)]


def _to_world(P, p):
    """rot_wc_ * p + cam_center_, rot_wc_ = rot_cw_^T (D5 item 1's order)"""
    P = [f64(v) for v in P]
    return [((P[i] * p[0] + P[3 + i] * p[1]) + P[6 + i] * p[2]) + P[12 + i] for i in range(3)]


def triangulate_pair(P1, P2, T, K, kl1, kl2, fin):
    """the stereo branch's algebra (frame.cc:1009-1104): the two planes, the Pluecker line, the trimmed end points in P1's frame"""
    z, one = f64(0.0), f64(1.0)
    g = lambda k, n: f64(f32(k[n]))
    xs1, xe1 = [g(kl1, "startPointX"), g(kl1, "startPointY"), one], [g(kl1, "endPointX"), g(kl1, "endPointY"), one]
    xs2, xe2 = [g(kl2, "startPointX"), g(kl2, "startPointY"), one], [g(kl2, "endPointX"), g(kl2, "endPointY"), one]
    line1, line2 = fin(_cross(xs1, xe1)), fin(_cross(xs2, xe2))
    p1, p2 = fin(_plane(P1, line1)), fin(_plane(P2, line2))
    Ls = [[p1[i] * p2[j] - p2[i] * p1[j] for j in range(4)] for i in range(4)]               # L_star
    d = fin([Ls[2][1], Ls[0][2], Ls[1][0]])                                                  # the entries the reference reads
    m = fin([Ls[0][3], Ls[1][3], Ls[2][3]])
    pk = m + d                                                                               # plucker_coord
    v = []
    for i in range(3):                                                                       # (transformation_line_cw * plucker).block<3,1>(0,0)
        s = T[i][0] * pk[0]
        for k in range(1, 6):
            s = s + T[i][k] * pk[k]
        v.append(s)
    fin(v)
    l1, l2, l3 = fin([(K[i][0] * v[0] + K[i][1] * v[1]) + K[i][2] * v[2] for i in range(3)])  # _K * (...)
    M = [[z, -m[2], m[1], d[0]], [m[2], z, -m[0], d[1]], [-m[1], m[0], z, d[2]], [-d[0], -d[1], -d[2], z]]
    out = []
    for px, py in ((g(kl1, "startPointX"), g(kl1, "startPointY")), (g(kl1, "endPointX"), g(kl1, "endPointY"))):
        xc = fin(-((py - (l2 / l1) * px) + (l3 / l2)) * ((l1 * l2) / (l1 * l1 + l2 * l2)))
        yc = fin(-(l1 / l2) * xc - (l3 / l2))
        y0 = fin(py - (l2 / l1) * px)
        lt = fin(_cross([xc, yc, one], [z, y0, one]))
        pt = fin(_plane(P1, lt))
        I = fin([((M[i][0] * pt[0] + M[i][1] * pt[1]) + M[i][2] * pt[2]) + M[i][3] * pt[3] for i in range(4)])
        out.append(fin([I[0] / I[3], I[1] / I[3], I[2] / I[3]]))
    return out


def keyline_3d(cam, setup_type, P, kl, depth_pair=None, good=-1, kl_right=None):
    """frame::triangulate_stereo_for_line for one key line -> (pos_w [6] f64, valid); cam: dict fx, fy, cx, cy, focal_x_baseline"""
    fx, fy, cx, cy, fxb = (f64(cam[k]) for k in ("fx", "fy", "cx", "cy", "focal_x_baseline"))
    zero = np.zeros(6, np.float64)
    fin = _Finite()
    with np.errstate(all="ignore"):
        if setup_type == RGBD:
            dsp, dep = f32(depth_pair[0]), f32(depth_pair[1])
            if not (f64(0.0) < f64(dsp) and f64(0.0) < f64(dep)):
                return zero, False
            fx_inv, fy_inv = f64(1.0) / fx, f64(1.0) / fy                                  # perspective.cc:42
            pts = []
            for xn, yn, dd in (("startPointX", "startPointY", dsp), ("endPointX", "endPointY", dep)):
                ux = fin(f32(((f64(f32(kl[xn])) - cx) * f64(dd)) * fx_inv))
                uy = fin(f32(((f64(f32(kl[yn])) - cy) * f64(dd)) * fy_inv))
                pts.append(fin(_to_world(P, [f64(ux), f64(uy), f64(dd)])))
            if not fin.ok:
                return zero, False
            return np.array(pts[0] + pts[1], np.float64), True
        if good < 0 or kl_right is None or good >= len(kl_right):
            return zero, False
        z, one = f64(0.0), f64(1.0)
        P1 = [[fx, z, cx, z], [z, fy, cy, z], [z, z, one, z]]
        P2 = [[fx, z, cx, -fxb], [z, fy, cy, z], [z, z, one, z]]
        T = [[one if k == i else z for k in range(6)] for i in range(3)]
        K = [[fy, z, z], [z, fx, z], [-fy * cx, -fx * cy, fx * fy]]
        sp, ep = triangulate_pair(P1, P2, T, K, kl, kl_right[good], fin)
        wsp, wep = fin(_to_world(P, sp)), fin(_to_world(P, ep))
        if not fin.ok:                                                                          # D7
            return zero, False
        if f64(0) < wsp[2] and f64(0) < wep[2]:                                                 # the world z (frame.cc:1109)
            return np.array(wsp + wep, np.float64), True
        return zero, False


def keylines_3d(cam, setup_type, P, kls, kl_depths=None, good_match=None, kl_right=None):
    """one frame -> (pos_w [n, 6] f64, valid [n] u8)"""
    n = len(kls)
    pos = np.zeros((n, 6), np.float64)
    valid = np.zeros(n, np.uint8)
    for j in range(n):
        pw, ok = keyline_3d(cam, setup_type, P, kls[j], None if kl_depths is None else kl_depths[j],
                            -1 if good_match is None else int(good_match[j]), kl_right)
        pos[j], valid[j] = pw, ok
    return pos, valid


# ---------------------------------------------------------------------------------------------------------------- synthetic geometry
def project(cam, P, X):
    """pinhole projection of world point X through pose row P (rot_cw, trans_cw): (u, v, z_c) in f64"""
    R = np.asarray(P[:9], np.float64).reshape(3, 3)
    t = np.asarray(P[9:12], np.float64)
    xc = R @ np.asarray(X, np.float64) + t
    return cam["fx"] * xc[0] / xc[2] + cam["cx"], cam["fy"] * xc[1] / xc[2] + cam["cy"], xc[2]


def make_keyline(kl_dtype, sx, sy, ex, ey):
    """a key line record with the fields the two loops read (angle as the LSD wrapper forms it, atan2 of the direction)"""
    k = np.zeros(1, kl_dtype)[0]
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = sx, sy, ex, ey
    k["angle"] = np.float32(np.arctan2(ey - sy, ex - sx))
    return k
