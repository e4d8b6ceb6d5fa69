"""CPU restatement of landmark::update_normal_and_depth (data/landmark.cc:249-295) and Line::update_information
(data/landmark_line.cc:311-352) as plp_landmark_geometry_* / plp_landmark_line_geometry_* define them: plain Python
f64 per landmark in the reference's order, numpy.float32 where the reference stores a float.  A pose is the 15-double row of plp_observe_args;
only its entries 12-14, cam_center, are read."""
import math

import numpy as np

f32 = np.float32
UPDATED, SKIPPED, NO_OBSERVATIONS, REF_NOT_OBSERVED, INDEX_RANGE, OCTAVE_RANGE = range(6)   # plp_landmark_geometry_status


def normalized(x, y, z):
    """Eigen 3.3 normalized(): v / sqrt(squaredNorm), a zero vector stays zero (D5 item 1)"""
    sq = (x * x + y * y) + z * z
    if sq > 0.0:
        s = math.sqrt(sq)
        return x / s, y / s, z / s
    return x, y, z


def norm(x, y, z):
    return math.sqrt((x * x + y * y) + z * z)


def unit_terms(pose, pos, kfs):
    """(pos_w_ - cam_center).normalized() of every observation, in list order (:274-281)"""
    p = [float(v) for v in pos]
    out = []
    for kf in kfs:
        c = pose[kf]
        out.append(normalized(p[0] - float(c[12]), p[1] - float(c[13]), p[2] - float(c[14])))
    return out


def sum_in_order(terms):
    """mean_normal = mean_normal + normal.normalized(), from Vec3_t::Zero() (:272, :279)"""
    sx = sy = sz = 0.0
    for ux, uy, uz in terms:
        sx, sy, sz = sx + ux, sy + uy, sz + uz
    return sx, sy, sz


def sum_pairwise(terms):
    """what a tree reduction would form instead: NOT the reference's sum (tests/test_landmark_geometry_cpu.py holds the scene to seeing it)"""
    if not terms:
        return 0.0, 0.0, 0.0
    t = [tuple(v) for v in terms]
    while len(t) > 1:
        t = [tuple(a + b for a, b in zip(t[i], t[i + 1])) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def valid_range(dist, sf_level, sf_last):
    """max_valid_dist_ = dist * scale_factor (f64 product stored to the float member), min_valid_dist_ = max_valid_dist_ / scale_factors_.at(n - 1)
    (float / float) -> (min, max)"""
    mx = f32(float(dist) * float(f32(sf_level)))
    return f32(mx / f32(sf_last)), mx


def _count(counts, cap, f):
    return cap if counts is None else min(max(int(counts[f]), 0), cap)


def update_normal_and_depth(pose, octaves, counts, scale_factors, pos, ref_kf, skip, kfs, idxs, summation=sum_in_order):
    """one point landmark -> (status, normal or None, min or None, max or None).  octaves [F][cap]; kfs / idxs: its observations in list order"""
    F, cap = len(pose), len(octaves[0]) if len(octaves) else 0
    if skip:
        return SKIPPED, None, None, None                       # :257-260
    if len(kfs) == 0:
        return NO_OBSERVATIONS, None, None, None               # :266-269
    ref = int(ref_kf)
    if not 0 <= ref < F or any(not 0 <= int(k) < F for k in kfs):
        return INDEX_RANGE, None, None, None
    s = summation(unit_terms(pose, pos, [int(k) for k in kfs]))
    where = [i for i, k in enumerate(kfs) if int(k) == ref]
    if not where:
        return REF_NOT_OBSERVED, None, None, None              # observations.at(ref_keyfrm) (:285)
    idx = int(idxs[where[0]])
    if not 0 <= idx < _count(counts, cap, ref):
        return INDEX_RANGE, None, None, None                   # undist_keypts_.at(idx)
    octave = int(octaves[ref][idx])
    if not 0 <= octave < len(scale_factors):
        return OCTAVE_RANGE, None, None, None                  # scale_factors_.at(scale_level) (:286)
    c = pose[ref]
    dist = norm(float(pos[0]) - float(c[12]), float(pos[1]) - float(c[13]), float(pos[2]) - float(c[14]))
    mn, mx = valid_range(dist, scale_factors[octave], scale_factors[len(scale_factors) - 1])
    return UPDATED, normalized(*s), mn, mx


def update_information(pose, octaves, counts, scale_factors, scale_factors_lsd, pos, ref_kf, skip, kfs, idxs):
    """one line landmark -> (status, min or None, max or None)"""
    F, cap = len(pose), len(octaves[0]) if len(octaves) else 0
    if skip:
        return SKIPPED, None, None                             # :324-325
    if len(kfs) == 0:
        return NO_OBSERVATIONS, None, None                     # :333-334
    ref = int(ref_kf)
    if not 0 <= ref < F or any(not 0 <= int(k) < F for k in kfs):
        return INDEX_RANGE, None, None
    where = [i for i, k in enumerate(kfs) if int(k) == ref]
    idx = int(idxs[where[0]]) if where else 0                  # observations[ref_kf]: operator[] default-constructs 0 (:343)
    if not 0 <= idx < _count(counts, cap, ref):
        return INDEX_RANGE, None, None
    level = int(octaves[ref][idx])
    nl = len(scale_factors_lsd)
    if not 0 <= level < nl:
        return OCTAVE_RANGE, None, None
    p = [float(v) for v in pos]
    c = pose[ref]
    mp = (0.5 * (p[0] + p[3]), 0.5 * (p[1] + p[4]), 0.5 * (p[2] + p[5]))                 # :339
    distance = norm(mp[0] - float(c[12]), mp[1] - float(c[13]), mp[2] - float(c[14]))   # :342
    mn, mx = valid_range(distance, scale_factors_lsd[level], scale_factors[nl - 1])     # :349-350: the ORB table at the LSD level count
    return UPDATED, mn, mx


def refresh(pose, octaves, counts, scale_factors, pos_w, ref_kf, skip, obs_offsets, obs_kf, obs_idx, scale_factors_lsd=None, out=None,
            summation=sum_in_order):
    """all landmarks, in the array form of the C ABI: dict(normal (points), min_dist, max_dist, status); rows that are not UPDATED keep the values
    of `out` (default 0).  scale_factors_lsd given = lines."""
    lines = scale_factors_lsd is not None
    L = len(pos_w)
    o = dict(min_dist=np.zeros(L, np.float32), max_dist=np.zeros(L, np.float32), status=np.zeros(L, np.uint8))
    if not lines:
        o["normal"] = np.zeros((L, 3), np.float64)
    if out is not None:
        o = {k: np.array(out[k], copy=True) for k in o}
    pose = [[float(v) for v in row] for row in np.asarray(pose, np.float64).reshape(-1, 15)]
    octaves = np.asarray(octaves).tolist()
    for l in range(L):
        b, e = int(obs_offsets[l]), int(obs_offsets[l + 1])
        sk = bool(skip[l]) if skip is not None else False
        if lines:
            st, mn, mx = update_information(pose, octaves, counts, scale_factors, scale_factors_lsd, pos_w[l], ref_kf[l], sk, obs_kf[b:e], obs_idx[b:e])
        else:
            st, n, mn, mx = update_normal_and_depth(pose, octaves, counts, scale_factors, pos_w[l], ref_kf[l], sk, obs_kf[b:e], obs_idx[b:e], summation)
        o["status"][l] = st
        if st == UPDATED:
            o["min_dist"][l], o["max_dist"][l] = mn, mx
            if not lines:
                o["normal"][l] = n
    return o
