"""Plain-Python restatement of DESIGN.md section 5, D25 (the line map update): endpoint_trimming with both acceptance rules and what its call sites do with
the result, the pose graph's line cloud (optimize/graph_optimizer.cc:352-403) and the loop adjuster's (module/loop_bundle_adjuster.cc:184-244).  Python
floats are IEEE doubles; every sum is written in the order csrc/line_update.hpp writes it, the zero terms included, with explicit loops."""
import numpy as np

import pose_optimizer_ref as D15

f32 = D15.f32
_div = D15._div
_sqrt = D15._sqrt

TRIM_DEPTH_POSITIVE, TRIM_MAX_CHANGE = 0, 1
TRIM_OK, TRIM_SKIPPED, TRIM_NO_REF, TRIM_NOT_OBSERVED, TRIM_INDEX_RANGE, TRIM_REJECTED = range(6)
CORRECT_LINE_OK, CORRECT_LINE_ERASED, CORRECT_LINE_NO_REF, CORRECT_LINE_NO_VERTEX = range(4)
LM_NO_REF, LM_OPTIMIZED, LM_MOVED, LM_ERASED = range(4)
KF_OPTIMIZED, KF_PROPAGATED = 1, 2
SENTINEL = dict(pos_w=-7.25, pluecker=-7.25, status=0xEE, erase=0x77)


# ---- the 6 x 6 matrix [s R, skew(t) R; 0, R] as a full list of rows
def transform6(R, t, s=None):
    """R: 9 floats row-major, t: 3 floats; s None: block(0,0) = R, else s * R"""
    tx, ty, tz = t
    T = [[0.0] * 6 for _ in range(6)]
    for c in range(3):
        r0, r1, r2 = R[c], R[3 + c], R[6 + c]
        for i, r in enumerate((r0, r1, r2)):
            T[i][c] = r if s is None else s * r
            T[3 + i][3 + c] = r
        T[0][3 + c] = (0.0 * r0 + (-tz) * r1) + ty * r2
        T[1][3 + c] = (tz * r0 + 0.0 * r1) + (-tx) * r2
        T[2][3 + c] = ((-ty) * r0 + tx * r1) + 0.0 * r2
    return T


def apply6(T, v, rows=6):
    o = []
    for i in range(rows):
        s = T[i][0] * v[0]
        for k in range(1, 6):
            s = s + T[i][k] * v[k]
        o.append(s)
    return o


def product6(X, Y):
    C = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(6):
            c = X[i][0] * Y[0][j]
            for k in range(1, 6):
                c = c + X[i][k] * Y[k][j]
            C[i][j] = c
    return C


def sim3_transform6(sim3):
    q = [float(v) for v in sim3]
    return transform6(D15.rot_from_quat(q[:4]), q[4:7], q[7])


# ---- line3d_trim (csrc/line3d.hpp, D7)
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def trim_point(P, M, l1, l2, l3, den, px, py):
    x, y = float(px), float(py)
    xc = -((y - _div(l2, l1) * x) + _div(l3, l2)) * _div(l1 * l2, den)
    yc = -_div(l1, l2) * xc - _div(l3, l2)
    y0 = y - _div(l2, l1) * x
    lt = _cross([xc, yc, 1.0], [0.0, y0, 1.0])
    pt = [(lt[0] * P[j] + lt[1] * P[4 + j]) + lt[2] * P[8 + j] for j in range(4)]
    I = [((M[4 * i] * pt[0] + M[4 * i + 1] * pt[1]) + M[4 * i + 2] * pt[2]) + M[4 * i + 3] * pt[3] for i in range(4)]
    return [_div(I[0], I[3]), _div(I[1], I[3]), _div(I[2], I[3])]


def reprojected_line(cam, pose, Lw):
    """(l1, l2, l3) of items 3-5: _K (transformation_line_cw L)(0..2)"""
    fx, fy, cx, cy = cam
    T = transform6(pose[:9], pose[9:12])
    v = apply6(T, Lw, 3)
    K = [fy, 0.0, 0.0, 0.0, fx, 0.0, -fy * cx, -fx * cy, fx * fy]
    return [(K[3 * i] * v[0] + K[3 * i + 1] * v[1]) + K[3 * i + 2] * v[2] for i in range(3)]


def trim_one(cam, pose, Lw, kl4, mode, old=None, median=None, max_change=0.1):
    """items 2-11 for one line against its reference key frame's pose row (>= 12 floats): (accepted, sp + ep)"""
    fx, fy, cx, cy = cam
    l1, l2, l3 = reprojected_line(cam, pose, Lw)
    den = l1 * l1 + l2 * l2
    P = [0.0] * 12
    for c in range(4):
        a0, a1, a2 = (pose[c], pose[3 + c], pose[6 + c]) if c < 3 else (pose[9], pose[10], pose[11])
        P[c] = (fx * a0 + 0.0 * a1) + cx * a2
        P[4 + c] = (0.0 * a0 + fy * a1) + cy * a2
        P[8 + c] = (0.0 * a0 + 0.0 * a1) + 1.0 * a2
    M = [0.0, -Lw[2], Lw[1], Lw[3],
         Lw[2], 0.0, -Lw[0], Lw[4],
         -Lw[1], Lw[0], 0.0, Lw[5],
         -Lw[3], -Lw[4], -Lw[5], 0.0]
    sp = trim_point(P, M, l1, l2, l3, den, kl4[0], kl4[1])
    ep = trim_point(P, M, l1, l2, l3, den, kl4[2], kl4[3])
    if mode == TRIM_MAX_CHANGE:
        med = float(f32(median))
        d = [sp[i] - old[i] for i in range(3)] + [ep[i] - old[3 + i] for i in range(3)]
        ds = _div(_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), med)
        de = _div(_sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]), med)
        return not (ds > max_change or de > max_change), sp + ep
    zs = ((pose[6] * sp[0] + pose[7] * sp[1]) + pose[8] * sp[2]) + pose[11] * 1.0
    ze = ((pose[6] * ep[0] + pose[7] * ep[1]) + pose[8] * ep[2]) + pose[11] * 1.0
    return (0.0 < zs and 0.0 < ze), sp + ep


def _rows(a, n):
    return [[float(v) for v in row] for row in np.asarray(a, np.float64).reshape(-1, n)]


def trim_line_endpoints(cam, pluecker, ref_kf, obs_offsets, obs_kf, obs_idx, pose, keylines, mode=TRIM_DEPTH_POSITIVE, skip=None, kf_erased=None, counts=None,
                        pos_w_old=None, median_depth=None, max_change=0.1, out=None):
    """the array form of plp_trim_line_endpoints_*: dict(pos_w, status, erase); slots that are not written keep the values of `out` (default: SENTINEL).
    keylines: (F, cap) KL_DTYPE; cam = (fx, fy, cx, cy); pose rows of any stride >= 12"""
    pk = _rows(pluecker, 6)
    L = len(pk)
    po = np.asarray(pose, np.float64)
    F = po.shape[0]
    po = [[float(v) for v in row] for row in po]
    cap = keylines.shape[1] if F else 0
    old = None if pos_w_old is None else _rows(pos_w_old, 6)
    o = dict(pos_w=np.full((L, 6), SENTINEL["pos_w"]), status=np.full(L, SENTINEL["status"], np.uint8), erase=np.full(L, SENTINEL["erase"], np.uint8))
    if out is not None:
        o = {k: np.array(out[k], copy=True) for k in o}
    for l in range(L):
        st, pts = TRIM_OK, None
        r = int(ref_kf[l])
        if skip is not None and skip[l]:
            st = TRIM_SKIPPED
        elif not 0 <= r < F or (kf_erased is not None and kf_erased[r]):
            st = TRIM_NO_REF
        else:
            idx = -1
            for t in range(int(obs_offsets[l]), int(obs_offsets[l + 1])):
                if int(obs_kf[t]) == r:
                    idx = int(obs_idx[t])
                    break
            cnt = cap if counts is None else min(max(int(counts[r]), 0), cap)
            if idx == -1:
                st = TRIM_NOT_OBSERVED
            elif not 0 <= idx < cnt:
                st = TRIM_INDEX_RANGE
            else:
                k = keylines[r, idx]
                kl4 = (k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"])
                ok, pts = trim_one(cam, po[r], pk[l], kl4, mode, None if old is None else old[l], None if median_depth is None else median_depth[r], max_change)
                st = TRIM_OK if ok else TRIM_REJECTED
        o["status"][l] = st
        o["erase"][l] = 1 if st in (TRIM_NOT_OBSERVED, TRIM_REJECTED) else 0
        if st == TRIM_OK:
            o["pos_w"][l] = pts
    return o


def correct_landmark_lines(pluecker, ref_kf, sim3_cw, corrected_wc, corr_kf=None, lm_erased=None, kf_erased=None, out=None):
    """the array form of plp_correct_landmark_lines_*: dict(pluecker, status)"""
    pk = _rows(pluecker, 6)
    L, F = len(pk), len(sim3_cw)
    o = dict(pluecker=np.full((L, 6), SENTINEL["pluecker"]), status=np.full(L, SENTINEL["status"], np.uint8))
    if out is not None:
        o = {k: np.array(out[k], copy=True) for k in o}

    def vertex(r):
        return 0 <= r < F and not (kf_erased is not None and kf_erased[r])
    for l in range(L):
        r = int(ref_kf[l])
        c = r if corr_kf is None else int(corr_kf[l])
        if lm_erased is not None and lm_erased[l]:
            o["status"][l] = CORRECT_LINE_ERASED
        elif not vertex(r):
            o["status"][l] = CORRECT_LINE_NO_REF
        elif not vertex(c):
            o["status"][l] = CORRECT_LINE_NO_VERTEX
        else:
            C = product6(sim3_transform6(corrected_wc[c]), sim3_transform6(sim3_cw[c]))
            o["pluecker"][l] = apply6(C, pk[l])
            o["status"][l] = CORRECT_LINE_OK
    return o


def loop_ba_propagate_lines(pose_after, pose_before, kf_status, pluecker, ref_kf, line_optimized=None, pluecker_after=None, lm_erased=None, out=None):
    """the array form of plp_loop_ba_propagate_lines_*: dict(pluecker, status)"""
    pk = _rows(pluecker, 6)
    pa, pb = _rows(pose_after, 15), _rows(pose_before, 12)
    L, F = len(pk), len(pa)
    o = dict(pluecker=np.full((L, 6), SENTINEL["pluecker"]), status=np.full(L, SENTINEL["status"], np.uint8))
    if out is not None:
        o = {k: np.array(out[k], copy=True) for k in o}
    for l in range(L):
        r = int(ref_kf[l])
        if lm_erased is not None and lm_erased[l]:
            o["status"][l] = LM_ERASED
        elif line_optimized is not None and line_optimized[l]:
            o["pluecker"][l] = np.asarray(pluecker_after, np.float64).reshape(-1, 6)[l]
            o["status"][l] = LM_OPTIMIZED
        elif not 0 <= r < F or int(kf_status[r]) not in (KF_OPTIMIZED, KF_PROPAGATED):
            o["status"][l] = LM_NO_REF
        else:
            b, a = pb[r], pa[r]
            Lc = apply6(transform6(b[:9], b[9:12]), pk[l])
            Rwc = [a[3 * j + i] for i in range(3) for j in range(3)]
            o["pluecker"][l] = apply6(transform6(Rwc, a[12:15]), Lc)
            o["status"][l] = LM_MOVED
    return o


def line_map_update(cam, pose, kf_erased, keylines, kl_counts, lines, mode, pluecker=None, moved=None, erase=None, median_depth=None, max_change=0.1,
                    scale_factors=None, scale_factors_lsd=None):
    """what line_map_update_step.run leaves in the tables (D25): the estimate taken where `moved`, the trim of those lines, the write-back under the status,
    the erased lines flagged, Line::update_information (tests/landmark_geometry_ref.py) -> dict of the tables and statuses"""
    import landmark_geometry_ref as LG
    pk, pos, skip = lines["pluecker_lines"].copy(), lines["pos_w_lines"].copy(), lines["skip_lines"].copy()
    L = len(pk)
    mv = np.ones(L, bool) if moved is None else np.asarray(moved).astype(bool)
    if pluecker is not None:
        pk[mv] = pluecker[mv]
    t = trim_line_endpoints(cam, pk, lines["ref_kf_lines"], lines["obs_offsets_lines"], lines["obs_kf_lines"], lines["obs_idx_lines"], pose, keylines, mode=mode,
                            skip=skip | (~mv).astype(np.uint8), kf_erased=kf_erased, counts=kl_counts, pos_w_old=pos if mode == TRIM_MAX_CHANGE else None,
                            median_depth=median_depth, max_change=max_change, out=dict(pos_w=pos, status=np.zeros(L, np.uint8), erase=np.zeros(L, np.uint8)))
    skip = skip | t["erase"] | (np.zeros(L, np.uint8) if erase is None else (np.asarray(erase) != 0).astype(np.uint8))
    g = LG.refresh(np.asarray(pose)[:, :15], keylines["octave"], kl_counts, scale_factors, t["pos_w"], lines["ref_kf_lines"], skip, lines["obs_offsets_lines"],
                   lines["obs_kf_lines"], lines["obs_idx_lines"], scale_factors_lsd=scale_factors_lsd,
                   out=dict(min_dist=lines.get("min_dist_lines", np.zeros(L, np.float32)), max_dist=lines.get("max_dist_lines", np.zeros(L, np.float32)),
                            status=np.zeros(L, np.uint8)))
    return dict(pluecker_lines=pk, pos_w_lines=t["pos_w"], skip_lines=skip, min_dist_lines=g["min_dist"], max_dist_lines=g["max_dist"], trim_status=t["status"],
                trim_erase=t["erase"], geometry_status_lines=g["status"])
