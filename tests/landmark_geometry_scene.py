"""The scene of the landmark-geometry tests (plp_landmark[_line]_geometry_*, landmark_refresh_step): F = 600 key frames looking along +z at a
cloud of about 700 point and 300 line landmarks, ragged observation lists in shuffled key-frame order whose lengths cycle through
0, 1, 2, 3, 5, 8, 63, 64, 65, 257 (around one and several tiles of the kernel), one landmark seen by every key frame, and one landmark of
every special kind (KINDS).  Built once per process; the restated tables are computed once and shared (want_points / want_lines)."""
import functools

import numpy as np

import landmark_geometry_ref as G
import landmark_observe_ref as R
from plp import plp

F, CAP = 600, 64
N_POINTS, N_LINES = 700, 300
OBS_COUNTS = (0, 1, 2, 3, 5, 8, 63, 64, 65, 257)
NUM_LEVELS, NUM_LEVELS_LSD = 8, 2
SENT_F32, SENT_F64, SENT_U8 = np.float32(-7.5), -3.25, np.uint8(0xEE)
# the first landmarks of both lists are the special ones, in this order (the rest are ordinary)
KINDS = ("all_keyframes", "skipped", "skipped_without_observations", "ref_first", "ref_last", "ref_missing", "on_camera_centre", "ref_kf_above_table",
         "ref_kf_negative", "obs_kf_above_table", "obs_kf_negative", "feature_index_at_count", "feature_index_negative", "octave_above_table",
         "octave_negative")


def _rot(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _lists(rng, n, special_first):
    """observation lists of n landmarks: (offsets, kf, idx filled later, ref_kf, skip, kind per landmark)"""
    kfs, ref, skip, kinds = [], np.zeros(n, np.int32), np.zeros(n, np.uint8), [None] * n
    for l in range(n):
        kind = KINDS[l] if l < len(KINDS) and special_first else None
        kinds[l] = kind
        cnt = OBS_COUNTS[l % len(OBS_COUNTS)]
        if kind == "all_keyframes":
            cnt = F
        elif kind == "skipped_without_observations":
            cnt = 0
        elif kind is not None:
            cnt = (5, 8, 63, 65)[l % 4]
        k = rng.permutation(F)[:cnt].astype(np.int32)           # at most one observation per key frame, shuffled key-frame order
        if cnt:
            r = int(k[rng.integers(0, cnt)])
            if kind == "ref_first":
                r = int(k[0])
            if kind == "ref_last":
                r = int(k[-1])
            if kind == "ref_missing":
                r = int(np.setdiff1d(np.arange(F), k)[0])
            ref[l] = r
        else:
            ref[l] = int(rng.integers(0, F))
        if kind in ("skipped", "skipped_without_observations") or (kind is None and rng.uniform() < 0.05):
            skip[l] = 1
        if kind == "ref_kf_above_table":
            ref[l] = F
        if kind == "ref_kf_negative":
            ref[l] = -1
        if kind == "obs_kf_above_table":
            k[len(k) // 2] = F
        if kind == "obs_kf_negative":
            k[0] = -3
        kfs.append(k)
    off = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.int32)
    return off, np.concatenate(kfs).astype(np.int32), ref, skip, kinds


@functools.lru_cache(maxsize=None)
def scene():
    rng = np.random.default_rng(20251017)
    sc = dict(F=F, cap=CAP)
    # key frames: a cloud of cameras around the origin, all looking roughly along +z
    pose = np.zeros((F, 15))
    for f in range(F):
        Rm = _rot(rng, float(rng.uniform(0, 0.25)))
        centre = rng.uniform(-2.0, 2.0, 3) * (1.0, 1.0, 0.5)
        pose[f] = R.frame_pose(Rm, -Rm @ centre)
    sc["pose"] = pose
    sc["scale_factors"] = R.scale_factors(1.2, NUM_LEVELS)
    sc["scale_factors_lsd"] = R.scale_factors(2.0, NUM_LEVELS_LSD)
    sc["kf_erased"] = (rng.uniform(size=F) < 0.1).astype(np.uint8)
    for name, n, dt, width, noct in (("points", N_POINTS, plp.KP_DTYPE, 3, NUM_LEVELS), ("lines", N_LINES, plp.KL_DTYPE, 6, NUM_LEVELS_LSD)):
        feats = np.zeros((F, CAP), dt)
        feats["octave"] = rng.integers(0, noct, (F, CAP))
        counts = rng.integers(40, CAP + 1, F).astype(np.int32)
        counts[rng.integers(0, F, 50)] = CAP
        desc = rng.integers(0, 256, (F, CAP, 32), dtype=np.uint8)
        off, kf, ref, skip, kinds = _lists(rng, n, True)
        idx = np.zeros(len(kf), np.int32)
        pos = np.zeros((n, width))
        for l in range(n):
            b, e = off[l], off[l + 1]
            p = rng.uniform(-3.0, 3.0, 3) + (0.0, 0.0, float(rng.uniform(6.0, 25.0)))
            pos[l, :3] = p
            if width == 6:
                pos[l, 3:] = p + rng.uniform(-1.0, 1.0, 3)
            for o in range(b, e):
                idx[o] = rng.integers(0, counts[kf[o]]) if 0 <= kf[o] < F else 0
            here = [o for o in range(b, e) if kf[o] == ref[l]]
            kind = kinds[l]
            if kind == "on_camera_centre":                       # the zero term: pos_w is one observing camera's centre, bit for bit
                pos[l, :3] = pose[kf[b + 1], 12:15]
                if width == 6:
                    pos[l, 3:] = pose[kf[b + 1], 12:15]
            if kind == "feature_index_at_count":
                counts[ref[l]] = 50
                idx[here[0]] = 50
            if kind == "feature_index_negative":
                idx[here[0]] = -1
            if kind == "octave_above_table":
                feats["octave"][ref[l], idx[here[0]]] = noct
            if kind == "octave_negative":
                feats["octave"][ref[l], idx[here[0]]] = -1
        if name == "lines":                                      # the idx = 0 fallback of a missing reference key frame must be told from any other slot
            l = kinds.index("ref_missing")
            feats["octave"][ref[l], 0] = 1
            feats["octave"][ref[l], 1:] = 0
        sc[name] = dict(feats=feats, counts=counts, desc=desc, pos_w=pos, ref_kf=ref, skip=skip, obs_offsets=off, obs_kf=kf, obs_idx=idx, kinds=kinds, L=n,
                        desc_lm=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    return sc


def sentinels(L, lines=False):
    o = dict(min_dist=np.full(L, SENT_F32, np.float32), max_dist=np.full(L, SENT_F32, np.float32), status=np.full(L, SENT_U8, np.uint8))
    if not lines:
        o["normal"] = np.full((L, 3), SENT_F64, np.float64)
    return o


def restate(sc, name, rows=None, summation=G.sum_in_order):
    """the restatement over the sentinel-filled outputs, for all landmarks or for the rows given"""
    t = sc[name]
    lines = name == "lines"
    rows = np.arange(t["L"]) if rows is None else np.asarray(rows)
    pos, ref, skip, off, kf, idx = sublist(t, rows)
    return G.refresh(sc["pose"], t["feats"]["octave"], t["counts"], sc["scale_factors"], pos, ref, skip, off, kf, idx,
                     scale_factors_lsd=sc["scale_factors_lsd"] if lines else None, out=sentinels(len(rows), lines), summation=summation)


@functools.lru_cache(maxsize=None)
def want_points():
    return restate(scene(), "points")


@functools.lru_cache(maxsize=None)
def want_lines():
    return restate(scene(), "lines")


def sublist(t, rows):
    """the landmarks `rows` of a table as a call of their own: (pos_w, ref_kf, skip, obs_offsets, obs_kf, obs_idx)"""
    rows = np.asarray(rows)
    off = np.concatenate([[0], np.cumsum(t["obs_offsets"][rows + 1] - t["obs_offsets"][rows])]).astype(np.int32)
    sel = np.concatenate([np.arange(t["obs_offsets"][l], t["obs_offsets"][l + 1]) for l in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    return t["pos_w"][rows], t["ref_kf"][rows], t["skip"][rows], off, t["obs_kf"][sel], t["obs_idx"][sel]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
