"""CPU restatement of the key-frame pair line triangulation (plp_median_depth_* / plp_triangulate_keyline_pairs_*):
mapping_module::triangulate_line_with_two_keyframes (mapping_module.cc:482-601; initializer.cc:585-667 is the same loop with other thresholds
and no duplicate check), module::two_view_triangulator_line::triangulate (two_view_triangulator_line.cc:52-296, .h:128-151) and
keyframe::compute_median_depth (data/keyframe.cc:825-857), written from the reference's sources with the numeric contract of DESIGN.md
section 5, D8.  It is a literal serial loop: neighbour after neighbour, match after match, the duplicate check reading what earlier
iterations wrote.  Not compiled from the reference (unpinned, like D5-D7).

A key frame is a dict: keylines (n records of plp.KL_DTYPE), line_functions (n, 3) f64, kl_x_right (n, 2) f32, kp_depths (k,) f32 (the KEY
POINTS' depths_), pose (15,) f64 (frame_pose), median_depth f32, lines_3d (n, 6) f64 or None, occupied (n,) u8."""
import math

import numpy as np

from landmark_observe_ref import frame_pose, reproject  # noqa: F401  (frame_pose re-exported for the tests)
from stereo_keylines_ref import _Finite, angle_deg, point_distance, triangulate_pair

f32, f64 = np.float32, np.float64
MONOCULAR, STEREO, RGBD = 0, 1, 2
(CREATED, GATE_DISTANCE, GATE_ENDPOINTS, GATE_ANGLE, OCCUPIED_CUR, OCCUPIED_NGH, NO_PARALLAX, TOO_CLOSE, TOO_LONG, DEPTH, REPROJ_MID,
 REPROJ_END, SCALE, NON_FINITE, KP_DEPTH_RANGE) = range(15)
STATUS_NAMES = ("CREATED", "GATE_DISTANCE", "GATE_ENDPOINTS", "GATE_ANGLE", "OCCUPIED_CUR", "OCCUPIED_NGH", "NO_PARALLAX", "TOO_CLOSE",
                "TOO_LONG", "DEPTH", "REPROJ_MID", "REPROJ_END", "SCALE", "NON_FINITE", "KP_DEPTH_RANGE")
MAPPING_GATES = dict(dist_thr=50.0, endpoint_thr=400.0, angle_thr=20.0, skip_occupied=1)       # mapping_module.cc:506, :529, :564
INITIALIZER_GATES = dict(dist_thr=30.0, endpoint_thr=200.0, angle_thr=5.0, skip_occupied=0)    # initializer.cc
CHI_SQ_2D = f32(5.99146)


# ---------------------------------------------------------------------------------------------------------------- median depth
def depth_of(pose, pos, abs_flag):
    """one entry of `depths` (keyframe.cc:839-851): the f64 sum with the FLOAT trans_cw_z, std::abs in f64, stored as float"""
    P = [f64(v) for v in pose]
    x, y, z = (f64(v) for v in pos)
    pos_c_z = ((P[6] * x + P[7] * y) + P[8] * z) + f64(f32(P[11]))
    if abs_flag:
        pos_c_z = abs(pos_c_z)
    d = f32(pos_c_z)
    return f32(0.0) if d == 0 else d            # a zero depth is +0.0 (D8): -0.0 and 0.0 tie in std::sort


def median_depth(pose, pos_w, valid, abs_flag):
    """keyframe::compute_median_depth(abs) -> (median f32, count); no landmark: (0.0, 0), where the reference throws"""
    depths = [depth_of(pose, pos_w[i], abs_flag) for i in range(len(pos_w)) if valid is None or valid[i]]
    if not depths:
        return f32(0.0), 0
    depths = np.sort(np.array(depths, np.float32))
    return depths[(len(depths) - 1) // 2], len(depths)


# ---------------------------------------------------------------------------------------------------------------- the gates
def gate(kl1, kl2, dist, dist_thr, endpoint_thr, angle_thr):
    """mapping_module.cc:506-533 -> CREATED (= passed) or the gate that stopped the match"""
    if not (f32(dist) < f32(dist_thr)):
        return GATE_DISTANCE
    ds = point_distance(f32(kl1["startPointX"]) - f32(kl2["startPointX"]), f32(kl1["startPointY"]) - f32(kl2["startPointY"]))
    de = point_distance(f32(kl1["endPointX"]) - f32(kl2["endPointX"]), f32(kl1["endPointY"]) - f32(kl2["endPointY"]))
    ang = angle_deg(kl1["angle"], kl2["angle"])
    if not (ds < f32(endpoint_thr) and de < f32(endpoint_thr)):
        return GATE_ENDPOINTS
    if not (ang < f32(angle_thr)):
        return GATE_ANGLE
    return CREATED


# ---------------------------------------------------------------------------------------------------------------- triangulate
def _bearing_w(cam, P, kl):
    """:68-85: the middle point's bearing, turned by rot_w? = rot_?w^T"""
    x = (f64(f32(kl["pt_x"])) - f64(cam["cx"])) / f64(cam["fx"])
    y = (f64(f32(kl["pt_y"])) - f64(cam["cy"])) / f64(cam["fy"])
    n = np.sqrt((x * x + y * y) + f64(1.0))
    c = [x / n, y / n, f64(1.0) / n]
    return [(P[i] * c[0] + P[3 + i] * c[1]) + P[6 + i] * c[2] for i in range(3)]


def _norm3(a, b):
    d = [a[i] - b[i] for i in range(3)]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def _rel_gap(a, b):
    m = max(abs(float(a)), abs(float(b)))
    return abs(float(a) - float(b)) / m if m > 0 else 0.0


def cos_parallax_thr(deg):
    """cos_rays_parallax_thr_: the float of cos(thr * M_PI / 180.0), thr a float (.cc:41, .h:112)"""
    return f32(math.cos(float(f32(deg)) * math.pi / 180.0))


def triangulate(cam, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, cos_thr, kf1, kf2, j, t, gaps=None):
    """two_view_triangulator_line::triangulate(idx_1 = j, idx_2 = t) -> (status, pos_w [6] or None, branch 1 / 2 / 3 or 0).
    gaps: a list that receives (kind, relative gap) of every comparison of two cosines where a libm result takes part."""
    with np.errstate(all="ignore"):
        kl1, kl2 = kf1["keylines"][j], kf2["keylines"][t]
        P1r, P2r = [f64(v) for v in kf1["pose"]], [f64(v) for v in kf2["pose"]]
        fx, fy, cx, cy = (f64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        xr1, xr2 = f32(kf1["kl_x_right"][j][0]), f32(kf2["kl_x_right"][t][0])
        s1, s2 = bool(f32(0) <= xr1), bool(f32(0) <= xr2)
        w1, w2 = _bearing_w(cam, P1r, kl1), _bearing_w(cam, P2r, kl2)
        cr = (w1[0] * w2[0] + w1[1] * w2[1]) + w1[2] * w2[2]
        half = f64(true_baseline) / f64(2.0)
        c1 = c2 = f64(2.0)
        d1 = d2 = None
        if s1:                                                  # depths_.at(idx_1): the key points' vector, a key-line index (D8 item 2)
            if j >= len(kf1["kp_depths"]):
                return KP_DEPTH_RANGE, None, 0
            d1 = f32(kf1["kp_depths"][j])
            c1 = f64(math.cos(2.0 * math.atan2(float(half), float(d1))))
        if s2:
            if t >= len(kf2["kp_depths"]):
                return KP_DEPTH_RANGE, None, 0
            d2 = f32(kf2["kp_depths"][t])
            c2 = f64(math.cos(2.0 * math.atan2(float(half), float(d2))))
        cs = c2 if c2 < c1 else c1                              # std::min
        if not (s1 or s2):
            two = bool(f64(0.0) < cr and cr < f64(cos_thr))
        else:
            two = bool(f64(0.0) < cr and cr < cs)
            if gaps is not None and f64(0.0) < cr:
                gaps.append(("rays", _rel_gap(cr, cs)))
        branch = 0
        if two:
            branch = 1
            z, one = f64(0.0), f64(1.0)
            Kc = [[fx, z, cx], [z, fy, cy], [z, z, one]]        # eigen_cam_matrix_
            Pm = []
            for Pr in (P1r, P2r):
                Tcw = [[Pr[3 * r + 0], Pr[3 * r + 1], Pr[3 * r + 2], Pr[9 + r]] for r in range(3)]
                Pm.append([[(Kc[i][0] * Tcw[0][c] + Kc[i][1] * Tcw[1][c]) + Kc[i][2] * Tcw[2][c] for c in range(4)] for i in range(3)])
            R = [[P1r[3 * r + c] for c in range(3)] for r in range(3)]
            tx, ty, tz = P1r[9], P1r[10], P1r[11]
            S = [[z, -tz, ty], [tz, z, -tx], [-ty, tx, z]]      # skew(trans_1w_)
            SR = [[(S[i][0] * R[0][c] + S[i][1] * R[1][c]) + S[i][2] * R[2][c] for c in range(3)] for i in range(3)]
            T = [R[i] + SR[i] for i in range(3)]
            K = [[fy, z, z], [z, fx, z], [-fy * cx, -fx * cy, fx * fy]]
            fin = _Finite()
            sp, ep = triangulate_pair(Pm[0], Pm[1], T, K, kl1, kl2, fin)
            if not fin.ok:
                return NON_FINITE, None, branch
        else:
            if gaps is not None and (s1 or s2):
                # :202 / :221 compare the two stereo cosines; equal depths give bit-identical sides on any libm
                kind = "stereo_equal_inputs" if (s1 and s2 and d1 == d2) else "stereo"
                gaps.append((kind, _rel_gap(c1, c2)))
            if s1 and c1 < c2:
                branch, row = 2, (None if kf1["lines_3d"] is None else kf1["lines_3d"][j])
            elif s2 and c2 < c1:
                branch, row = 3, (None if kf2["lines_3d"] is None else kf2["lines_3d"][t])
            else:
                return NO_PARALLAX, None, 0
            if setup_type == MONOCULAR or row is None:          # the reference leaves sp_3D / ep_3D unset here: no landmark (D8 item 4)
                return NO_PARALLAX, None, 0
            sp, ep = [f64(v) for v in row[:3]], [f64(v) for v in row[3:]]
        if not np.all(np.isfinite(sp + ep)):
            return NON_FINITE, None, branch
        cc1, cc2 = P1r[12:15], P2r[12:15]
        med = f64(f32(kf2["median_depth"]))                     # key frame 2's, three times (:246-253)
        if _norm3(sp, cc1) / med < f64(0.3) or _norm3(ep, cc2) / med < f64(0.3):
            return TOO_CLOSE, None, branch
        if _norm3(ep, sp) / med > f64(0.9):
            return TOO_LONG, None, branch
        for p in (sp, ep):
            for Pr in (P1r, P2r):
                if not (0 < ((Pr[6] * p[0] + Pr[7] * p[1]) + Pr[8] * p[2]) + Pr[11]):
                    return DEPTH, None, branch
        mid = [f64(0.5) * (sp[i] + ep[i]) for i in range(3)]
        sig1 = f32(level_sigma_sq[int(kl1["octave"])])
        sig2 = f32(level_sigma_sq[int(kl2["octave"])])
        for Pr, kl, sig in ((P1r, kl1, sig1), (P2r, kl2, sig2)):
            wrote, _, u, v, _ = reproject(cam, (0, 0, 0, 0), Pr, *mid)
            if not wrote:                                       # z <= 0 by rounding: the reference reads an unset Vec2_t (D8 item 5)
                return REPROJ_MID, None, branch
            ex, ey = f64(u) - f64(f32(kl["pt_x"])), f64(v) - f64(f32(kl["pt_y"]))
            sq = ex * ex + ey * ey
            if not np.isfinite(sq):
                return NON_FINITE, None, branch
            if f64(f32(CHI_SQ_2D * sig)) < sq:
                return REPROJ_MID, None, branch
        for Pr, fn, sig in ((P1r, kf1["line_functions"][j], sig1), (P2r, kf2["line_functions"][t], sig2)):
            l0, l1, l2 = (f64(v) for v in fn)
            for p in (sp, ep):
                wrote, _, u, v, _ = reproject(cam, (0, 0, 0, 0), Pr, *p)
                assert wrote                                    # the four depths were just found positive by the same sum
                err = f32(((l0 * f64(u) + l1 * f64(v)) + l2) / np.sqrt(l0 * l0 + l1 * l1))
                if not np.isfinite(err):
                    return NON_FINITE, None, branch
                if f32(CHI_SQ_2D * sig) < f32(abs(err)):        # no square, as written (:313-316)
                    return REPROJ_END, None, branch
        sf1, sf2 = f32(scale_factors[int(kl1["octave"])]), f32(scale_factors[int(kl2["octave"])])
        ratio_factor = f32(f32(2.0) * f32(scale_factor))        # 2.0f * max(scale_factor_, scale_factor_)
        for p in (sp, ep):
            da, db = _norm3(p, cc1), _norm3(p, cc2)
            if da == 0 or db == 0:
                return SCALE, None, branch
            ratio_dists = db / da
            ratio_octave = f32(sf1 / sf2)
            if not (f64(ratio_octave) / ratio_dists < f64(ratio_factor) and ratio_dists / f64(ratio_octave) < f64(ratio_factor)):
                return SCALE, None, branch
        return CREATED, np.array(sp + ep, np.float64), branch


# ---------------------------------------------------------------------------------------------------------------- the loop
def triangulate_group(cam, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr, gates, kfs, kf1,
                      neighbours, matches, gaps=None, info=None):
    """triangulate_line_with_two_keyframes(cur = kfs[kf1], ngh) for every ngh of `neighbours`, in order.  matches[k] = (train_idx, dist) of
    the 1-NN cur -> neighbours[k].  Landmarks created on the way are seen by the later iterations: occupancy is copied from the key frames'
    `occupied` and updated as the reference's add_landmark_line does.  Returns (out_match, out_pos_w, out_status) lists per neighbour and
    cur's occupancy after the group.  info: receives per neighbour a list of (slot, cause) for the OCCUPIED statuses ("input", "earlier
    neighbour", "earlier winner") and the branch of every CREATED."""
    cur = kfs[kf1]
    n = len(cur["keylines"])
    cos_thr = cos_parallax_thr(rays_parallax_deg_thr)
    occ_cur = np.array(cur["occupied"][:n], np.uint8).copy()
    taken_here = np.zeros(n, bool)
    out_m, out_p, out_s = [], [], []
    for k, kf2 in enumerate(neighbours):
        ngh = kfs[kf2]
        n2 = len(ngh["keylines"])
        occ_ngh = np.array(ngh["occupied"][:n2], np.uint8).copy()
        taken_ngh = np.zeros(n2, bool)
        tidx, dist = matches[k]
        om, op, os_ = np.full(n, -1, np.int32), np.zeros((n, 6), np.float64), np.zeros(n, np.uint8)
        notes = []
        for j in range(n):                                      # lsd_matches is in query order, one DMatch per query
            t = int(tidx[j])
            if n2 == 0 or not (0 <= t < n2):
                os_[j] = GATE_DISTANCE
                continue
            g = gate(cur["keylines"][j], ngh["keylines"][t], dist[j], gates["dist_thr"], gates["endpoint_thr"], gates["angle_thr"])
            if g != CREATED:
                os_[j] = g
                continue
            if gates["skip_occupied"]:                          # avoid duplicate triangulation (:564)
                if occ_cur[j]:
                    os_[j] = OCCUPIED_CUR
                    notes.append((j, "earlier neighbour" if taken_here[j] else "input"))
                    continue
                if occ_ngh[t]:
                    os_[j] = OCCUPIED_NGH
                    notes.append((j, "earlier winner" if taken_ngh[t] else "input"))
                    continue
            st, pos, branch = triangulate(cam, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, cos_thr, cur, ngh, j, t,
                                          gaps)
            os_[j] = st
            if st == CREATED:
                om[j], op[j] = t, pos
                occ_cur[j], occ_ngh[t] = 1, 1                   # add_landmark_line on both key frames (:581-582)
                taken_here[j], taken_ngh[t] = True, True
                notes.append((j, f"branch {branch}"))
        out_m.append(om); out_p.append(op); out_s.append(os_)
        if info is not None:
            info.append(notes)
    return out_m, out_p, out_s, occ_cur
