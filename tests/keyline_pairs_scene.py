"""Synthetic scenes with ground truth for the key-frame pair line triangulation tests (CPU and GPU use the same inputs, so what the CPU tests
assert about the restatement's output -- every status reached, the near ties of the parallax comparisons -- holds for the GPU comparison).

A scene: random 3-D segments in front of a rig of key frames with real poses, projected with the perspective restatement, the end points
perturbed by fractions of a pixel, slots shuffled per key frame, synthetic 256-bit LBD codes (a per-segment code with a few bits flipped per
view; some segments share a code, so that the 1-NN also returns wrong pairings), some key lines duplicated inside a key frame (several
queries then share a train index).  Key frame 0 has the identity pose; the last key frame is empty; one key frame stands far behind the rig
(scale check); one has fewer key points than key lines (depths_.at throws); pairs of key frames a few centimetres apart have less parallax
than the stereo baseline (the two stereo / RGB-D branches)."""
import importlib

import numpy as np

import keyline_pairs_ref as KP
import stereo_keylines_ref as SK

plp = importlib.import_module("structure-plp-slam_amd")
f32, f64 = np.float32, np.float64
CAM = dict(model="perspective", cols=640, rows=480, fx=500.0, fy=500.0, cx=320.0, cy=240.0, focal_x_baseline=50.0)
TRUE_BASELINE = 0.1
NUM_LEVELS, SCALE_FACTOR = 8, 1.2
CAP = 64
SENT_I32, SENT_U8, SENT_F64 = -77, 0xEE, -12345.5


def scale_tables():
    from landmark_observe_ref import scale_factors
    sf = scale_factors(SCALE_FACTOR, NUM_LEVELS)
    return sf, (sf * sf).astype(np.float32)                     # level_sigma_sq_ = scale_factors_^2 (orb_params::calc_level_sigma_sq)


def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _pose(rng, k, F):
    """key frame k's (R, camera centre): 0 = identity; odd ones a few centimetres from their predecessor; F - 2 far behind the rig"""
    if k == 0:
        return np.eye(3), np.zeros(3)
    if k == F - 2:
        return _rot(rng.normal(size=3) * 0.02), np.array([1.5, 0.3, -9.0])
    return _rot(rng.normal(size=3) * 0.05), rng.uniform(-0.8, 0.8, 3) * np.array([1.0, 0.5, 0.4])


def _segments(rng, n, n_long):
    segs = []
    for i in range(n):
        mid = np.array([rng.uniform(-2.2, 2.2), rng.uniform(-1.6, 1.6), rng.uniform(3.0, 8.0)])
        d = rng.normal(size=3) * np.array([1.0, 1.0, 0.15])     # mostly fronto-parallel: the 3-D midpoint then projects near the 2-D one
        d /= np.linalg.norm(d)
        half = rng.uniform(0.15, 0.6) if i >= n_long else rng.uniform(2.4, 3.0)
        if i < n_long:
            mid = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(5.5, 7.0)])
            d = np.array([np.cos(0.3 * i), np.sin(0.3 * i), 0.0])
        segs.append((mid - half * d, mid + half * d))
    return segs


def _keyline(sx, sy, ex, ey, octave):
    k = np.zeros(1, plp.KL_DTYPE)[0]
    sx, sy, ex, ey = f32(sx), f32(sy), f32(ex), f32(ey)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = sx, sy, ex, ey
    k["sPointInOctaveX"], k["sPointInOctaveY"], k["ePointInOctaveX"], k["ePointInOctaveY"] = sx, sy, ex, ey
    k["pt_x"], k["pt_y"] = (sx + ex) / f32(2), (sy + ey) / f32(2)
    k["angle"] = f32(np.arctan2(f64(ey) - f64(sy), f64(ex) - f64(sx)))
    k["octave"] = octave
    k["lineLength"] = f32(np.hypot(f64(ex) - f64(sx), f64(ey) - f64(sy)))
    k["response"], k["size"], k["numOfPixels"] = 1.0, 1.0, int(k["lineLength"]) + 1
    return k


def _line_function(kl):
    """the line through the two end points, (a, b, c) with a x + b y + c = 0"""
    s = [f64(kl["startPointX"]), f64(kl["startPointY"]), f64(1)]
    e = [f64(kl["endPointX"]), f64(kl["endPointY"]), f64(1)]
    return np.array(SK._cross(s, e), np.float64)


def nn_brute(q, t):
    """the 1-NN by brute force (first nearest; nothing within 128 -> (-1, 256))"""
    idx, dist = np.full(len(q), -1, np.int32), np.full(len(q), 256, np.int32)
    if len(t) == 0:
        return idx, dist
    tb = np.unpackbits(t, axis=1).astype(np.int16)
    for j in range(len(q)):
        d = np.abs(np.unpackbits(q[j])[None].astype(np.int16) - tb).sum(1)
        b = int(np.argmin(d))
        if d[b] <= 128:
            idx[j], dist[j] = b, d[b]
    return idx, dist


def make_scene(seed, setup_type, F=12, n_seg=44, n_long=4, perturb=0.3, extra_horizontal=False, few_keypoints=True, occupied_rate=0.08, cap=CAP,
               counts=None, n_keypoints=None):
    """-> dict(cam, kfs: the restatement's key-frame dicts, seg: per key frame the segment of every slot, segments, lbd: per key frame (n, 32)).
    cap: the slots of the table the scene is made for; counts: per key frame the largest number of key lines (None: cap); n_keypoints: a
    dict key frame -> the number of its key points (the others: 40 more than key lines)."""
    rng = np.random.default_rng(seed)
    segs = _segments(rng, n_seg, n_long)
    if extra_horizontal:                                        # exactly horizontal in key frame 0: reprojected l1 == 0 (NON_FINITE)
        for y in (-0.4, 0.2, 0.7):
            segs.append((np.array([-0.6, y, 5.0]), np.array([0.5, y, 5.0])))
    codes = rng.integers(0, 256, (len(segs), 32), dtype=np.uint8)
    for i in range(n_long + 2, len(segs), 7):                   # shared codes: wrong pairings for the gates and the geometry checks
        codes[i] = codes[i - 1]
    cloud = np.concatenate([np.array(s) for s in segs] + [rng.uniform([-3, -2, 2.5], [3, 2, 9], (60, 3))])
    kfs, seg_of, lbds = [], [], []
    prev = None
    for k in range(F):
        R, c = _pose(rng, k, F)
        if k % 2 == 1 and k < F - 2 and prev is not None:       # a few centimetres from the predecessor: less parallax than the baseline
            R, c = prev[0] @ _rot(rng.normal(size=3) * 0.002), prev[1] + rng.normal(size=3) * 0.012
        prev = (R, c)
        P = SK.frame_pose(R, -R @ c)
        rows = []
        if k != F - 1:                                          # the last key frame has no key line
            for i, (a, b) in enumerate(segs):
                ua, va, za = SK.project(CAM, P, a)
                ub, vb, zb = SK.project(CAM, P, b)
                if za <= 0.3 or zb <= 0.3 or not all(0 <= u < 640 for u in (ua, ub)) or not all(0 <= v < 480 for v in (va, vb)):
                    continue
                horiz = extra_horizontal and i >= len(segs) - 3
                for copy in range(2 if (rng.random() < 0.18 and not horiz) else 1):
                    n4 = np.zeros(4) if (perturb == 0 or horiz) else rng.normal(size=4) * perturb
                    if rng.random() < 0.06 and perturb:         # a badly localised end point now and then
                        n4 = n4 + rng.normal(size=4) * 4.0
                    ends = [ua + n4[0], va + n4[1], ub + n4[2], vb + n4[3]]
                    if rng.random() < 0.06 and perturb and not horiz:   # turned about its middle by 6-12 degrees: the middle still fits, the ends do not
                        th = np.deg2rad(rng.uniform(6, 12)) * rng.choice([-1, 1])
                        mx, my = (ends[0] + ends[2]) / 2, (ends[1] + ends[3]) / 2
                        hx, hy = (ends[2] - ends[0]) / 2, (ends[3] - ends[1]) / 2
                        rx, ry = np.cos(th) * hx - np.sin(th) * hy, np.sin(th) * hx + np.cos(th) * hy
                        ends = [mx - rx, my - ry, mx + rx, my + ry]
                    code = codes[i].copy()
                    flips = rng.choice(256, rng.integers(0, 7), replace=False)
                    for bit in flips:
                        code[bit // 8] ^= np.uint8(1 << (bit % 8))
                    rows.append((i, ends[0], ends[1], ends[2], ends[3], za, zb, code))
        order = rng.permutation(len(rows))[:cap if counts is None else min(int(counts[k]), cap)]
        rows = [rows[o] for o in order]
        n = len(rows)
        octs = rng.integers(0, 3, n)
        kls = np.zeros(n, plp.KL_DTYPE)
        for s, r in enumerate(rows):
            kls[s] = _keyline(r[1], r[2], r[3], r[4], int(octs[s]))
        fn = np.array([_line_function(kls[s]) for s in range(n)], np.float64).reshape(n, 3)
        xr = np.full((n, 2), -1.0, np.float32)
        kd = np.full((n, 2), -1.0, np.float32)
        lines_3d = None
        if setup_type == KP.RGBD:
            for s, r in enumerate(rows):
                if rng.random() < 0.8:                          # both end points have a depth
                    kd[s] = (f32(r[5] * (1 + rng.normal() * 0.002 * bool(perturb))), f32(r[6] * (1 + rng.normal() * 0.002 * bool(perturb))))
                    xr[s] = (f32(f64(kls[s]["startPointX"]) - CAM["focal_x_baseline"] / f64(kd[s][0])),
                             f32(f64(kls[s]["endPointX"]) - CAM["focal_x_baseline"] / f64(kd[s][1])))
            lines_3d, _ = SK.keylines_3d(CAM, SK.RGBD, P, kls, kl_depths=kd)
        klr, good = None, None
        if setup_type == KP.STEREO:
            klr = np.zeros(n, plp.KL_DTYPE)
            good = np.full(n, -1, np.int32)
            for s, r in enumerate(rows):
                nr = rng.normal(size=2) * 0.15 * bool(perturb)
                klr[s] = _keyline(f64(kls[s]["startPointX"]) - CAM["focal_x_baseline"] / r[5] + nr[0], kls[s]["startPointY"],
                                  f64(kls[s]["endPointX"]) - CAM["focal_x_baseline"] / r[6] + nr[1], kls[s]["endPointY"], int(octs[s]))
                if rng.random() < 0.8:
                    good[s] = s
                    xr[s] = (1.0, 1.0)                          # what the stereo constructor's association leaves (frame.cc:389-427)
            lines_3d, _ = SK.keylines_3d(CAM, SK.STEREO, P, kls, good_match=good, kl_right=klr)
        n_kp = n + 40
        if few_keypoints and k == 4:
            n_kp = max(n - 9, 0)                                # fewer key points than key lines: depths_.at(idx) throws for the last slots
        if n_keypoints is not None and k in n_keypoints:
            n_kp = int(n_keypoints[k])
        kp_depths = rng.uniform(2.0, 10.0, n_kp).astype(np.float32)
        if k % 3 == 0 and n_kp > 6:
            kp_depths[3:6] = kp_depths[2]                       # equal depths: both stereo cosines from bit-identical inputs
        zc = (cloud - c) @ R.T
        valid = (zc[:, 2] > 0.1).astype(np.uint8)
        med, _ = KP.median_depth(P, cloud, valid, True)
        occ = (rng.random(n) < occupied_rate).astype(np.uint8)
        kfs.append(dict(keylines=kls, line_functions=fn, kl_x_right=xr, kl_depths=kd, kp_depths=kp_depths, pose=P, median_depth=med,
                        lines_3d=lines_3d, occupied=occ, keylines_right=klr, good_match=good, cloud=cloud, cloud_valid=valid))
        seg_of.append([r[0] for r in rows])
        lbds.append(np.array([r[7] for r in rows], np.uint8).reshape(n, 32))
    return dict(cam=CAM, setup_type=setup_type, kfs=kfs, seg=seg_of, segments=segs, lbd=lbds, F=F)


def make_groups(seed, F, G=9):
    """G groups of 3-10 neighbours; every key frame is cur once or more, the empty one and the far one included"""
    rng = np.random.default_rng(seed + 1000)
    groups = []
    for g in range(G):
        kf1 = [0, 2, F - 2, 4, 1, 6, F - 1, 3, 8][g % 9] % F
        others = [k for k in range(F) if k != kf1]
        size = int(rng.integers(3, min(10, len(others)) + 1))
        ngh = [int(k) for k in rng.permutation(others)[:size]]
        if kf1 % 2 == 0 and kf1 + 1 < F - 2 and kf1 + 1 not in ngh:
            ngh[0] = kf1 + 1                                    # its low-parallax partner
        groups.append((kf1, ngh))
    return groups


def match_all(scene, groups):
    """the brute-force 1-NN cur -> ngh of every pair, in group order: list per group of [(train_idx, dist), ...]"""
    return [[nn_brute(scene["lbd"][kf1], scene["lbd"][kf2]) for kf2 in ngh] for kf1, ngh in groups]


def run_ref(scene, groups, matches, gates, gaps=None, info=None, occupied=None, cap=CAP):
    """the restatement over every group -> (match, pos_w, status) in the (P, cap) layout with the sentinels in the slots it does not write,
    occupied_cur (G, cap); info: per pair the restatement's notes"""
    sf, ls = scale_tables()
    P = sum(len(n) for _, n in groups)
    om = np.full((P, cap), SENT_I32, np.int32)
    op = np.full((P, cap, 6), SENT_F64, np.float64)
    os_ = np.full((P, cap), SENT_U8, np.uint8)
    oc = np.full((len(groups), cap), SENT_U8, np.uint8)
    kfs = scene["kfs"]
    if occupied is not None:
        kfs = [dict(kf, occupied=occupied[k][:len(kf["keylines"])]) for k, kf in enumerate(kfs)]
    p = 0
    for g, (kf1, ngh) in enumerate(groups):
        notes = [] if info is not None else None
        m, pw, st, occ = KP.triangulate_group(scene["cam"], scene["setup_type"], TRUE_BASELINE, sf, ls, SCALE_FACTOR, 1.0, gates, kfs, kf1, ngh,
                                              matches[g], gaps, notes)
        n = len(kfs[kf1]["keylines"])
        for k in range(len(ngh)):
            om[p, :n], op[p, :n], os_[p, :n] = m[k], pw[k], st[k]
            if info is not None:
                info.append(notes[k])
            p += 1
        oc[g, :n] = occ
    return om, op, os_, oc


def table(scene, occupied=None, cap=CAP):
    """the key-frame table as the (F, cap, ...) arrays of plp_keyline_pairs_args; slots past the counts hold values that must not be read"""
    F, kfs = scene["F"], scene["kfs"]
    kp_cap = max(len(kf["kp_depths"]) for kf in kfs)
    t = dict(keylines=np.zeros((F, cap), plp.KL_DTYPE), counts=np.zeros(F, np.int32), line_functions=np.full((F, cap, 3), np.nan),
             kl_x_right=np.full((F, cap, 2), 5.0, np.float32), kp_depths=np.full((F, kp_cap), np.nan, np.float32), kp_counts=np.zeros(F, np.int32),
             pose=np.zeros((F, 15)), median_depth=np.zeros(F, np.float32), occupied=np.ones((F, cap), np.uint8),
             lines_3d=None if scene["setup_type"] == KP.MONOCULAR else np.full((F, cap, 6), np.nan), lbd=np.zeros((F, cap, 32), np.uint8))
    t["keylines"]["startPointX"] = np.nan
    for k, kf in enumerate(kfs):
        n = len(kf["keylines"])
        t["counts"][k], t["kp_counts"][k] = n, len(kf["kp_depths"])
        t["keylines"][k, :n], t["line_functions"][k, :n], t["kl_x_right"][k, :n] = kf["keylines"], kf["line_functions"], kf["kl_x_right"]
        t["kp_depths"][k, :len(kf["kp_depths"])] = kf["kp_depths"]
        t["pose"][k], t["median_depth"][k] = kf["pose"], kf["median_depth"]
        t["occupied"][k, :n] = kf["occupied"] if occupied is None else occupied[k][:n]
        t["lbd"][k, :n] = scene["lbd"][k]
        if t["lines_3d"] is not None:
            t["lines_3d"][k, :n] = kf["lines_3d"]
    return t


def flat_matches(groups, matches, cap=CAP):
    """(train_idx, dist) as (P, cap) arrays; slots past cur's count hold an index that would be out of bounds if it were followed"""
    P = sum(len(n) for _, n in groups)
    ti, di = np.full((P, cap), 1 << 20, np.int32), np.zeros((P, cap), np.int32)
    p = 0
    for g, (_, ngh) in enumerate(groups):
        for k in range(len(ngh)):
            a, b = matches[g][k]
            ti[p, :len(a)], di[p, :len(a)] = a, b
            p += 1
    return ti, di


# the scenes of the parity tests: (name, seed, setup type, gates); tuned on the restatement's output (tests/test_keyline_pairs_cpu.py)
SCENES = [("mono-mapping", 11, KP.MONOCULAR, KP.MAPPING_GATES), ("mono-init", 12, KP.MONOCULAR, KP.INITIALIZER_GATES),
          ("rgbd-mapping", 13, KP.RGBD, KP.MAPPING_GATES), ("rgbd-init", 14, KP.RGBD, KP.INITIALIZER_GATES),
          ("stereo-mapping", 15, KP.STEREO, KP.MAPPING_GATES), ("stereo-init", 16, KP.STEREO, KP.INITIALIZER_GATES)]

_cache = {}


def scene_case(name):
    """-> (scene, groups, matches, gates, reference outputs, gaps, info), computed once per process"""
    if name not in _cache:
        _, seed, setup, gates = next(s for s in SCENES if s[0] == name)
        scene = make_scene(seed, setup)
        groups = make_groups(seed, scene["F"])
        matches = match_all(scene, groups)
        gaps, info = [], []
        ref = run_ref(scene, groups, matches, gates, gaps, info)
        _cache[name] = (scene, groups, matches, gates, ref, gaps, info)
    return _cache[name]


# ------------------------------------------------------------------------------------------ above one workgroup of slots (256 query slots)
# The scenes of tests/test_gpu_pair_kernels_wide.py; what they are named for is asserted on the restatement in tests/test_pair_kernels_wide_cpu.py.
WIDE_CAP = 300                                                  # two trips of the resolve kernel's loops, the second with 44 slots
LIMIT_CAP = 8192                                                # the largest capacity the entries accept: 40 960 B of dynamic LDS
NO_GATES_CHECK = dict(KP.MAPPING_GATES, skip_occupied=0)        # the mapping thresholds without the duplicate check
_SLOT_FIELDS = ("keylines", "line_functions", "kl_x_right", "kl_depths", "lines_3d", "occupied")


def _reindex(scene, k, index):
    """key frame k's key lines become the old ones at `index` (monocular scenes: nothing refers to a slot by its number)"""
    assert scene["setup_type"] == KP.MONOCULAR
    kf = scene["kfs"][k]
    for f in _SLOT_FIELDS:
        if kf[f] is not None:
            kf[f] = kf[f][index].copy()
    scene["lbd"][k] = scene["lbd"][k][index].copy()
    scene["seg"][k] = [scene["seg"][k][i] for i in index]


def copy_slot(scene, k, src, dst):
    index = np.arange(len(scene["kfs"][k]["keylines"]))
    index[dst] = src
    _reindex(scene, k, index)


def swap_slots(scene, k, a, b):
    index = np.arange(len(scene["kfs"][k]["keylines"]))
    index[[a, b]] = index[[b, a]]
    _reindex(scene, k, index)


def tile_key_frame(scene, k, count):
    """repeat key frame k's key lines in turn until it has `count` of them"""
    _reindex(scene, k, np.arange(count) % len(scene["kfs"][k]["keylines"]))


def created_alone(scene, kf1, kf2, j, t, gates=KP.MAPPING_GATES, dist=7):
    """does query slot j of kf1 with train index t of kf2 pass the three gates and become a landmark when nothing is occupied?"""
    a, b = scene["kfs"][kf1], scene["kfs"][kf2]
    if KP.gate(a["keylines"][j], b["keylines"][t], dist, gates["dist_thr"], gates["endpoint_thr"], gates["angle_thr"]) != KP.CREATED:
        return False
    sf, ls = scale_tables()
    return KP.triangulate(scene["cam"], scene["setup_type"], TRUE_BASELINE, sf, ls, SCALE_FACTOR, KP.cos_parallax_thr(1.0), a, b, j, t)[0] == KP.CREATED


def plant_shared_train(scene, cur, neighbours, query_slots, train_slots, dist=7):
    """Key lines whose query slots share one train index: a segment that cur and every neighbour see, and that is triangulated into a landmark
    with each of them, is put into every slot of query_slots of cur (copies of one key line) and into slot train_slots[k] of neighbours[k].
    -> matches of the group (the brute-force 1-NN of the scene after the move; the planted queries name the planted train index with
    distance `dist`, every other query that named it is left without a match)"""
    segs = [scene["seg"][k] for k in neighbours]
    for j, s in enumerate(scene["seg"][cur]):
        if j in query_slots or not all(s in sg for sg in segs):
            continue
        ts = [sg.index(s) for sg in segs]
        if any(t in train_slots for t in ts) or not all(created_alone(scene, cur, k, j, t, dist=dist) for k, t in zip(neighbours, ts)):
            continue
        for q in query_slots:
            copy_slot(scene, cur, j, q)
        for k, t, to in zip(neighbours, ts, train_slots):
            swap_slots(scene, k, t, to)
        break
    else:
        raise AssertionError("no segment of this scene is triangulated with every neighbour")
    matches = []
    for k, to in zip(neighbours, train_slots):
        ti, di = nn_brute(scene["lbd"][cur], scene["lbd"][k])
        ti[ti == to], di[ti == to] = -1, 256
        ti[list(query_slots)], di[list(query_slots)] = to, dist
        matches.append((ti, di))
    return matches


_wide = {}


def wide_counts_case():
    """L1: cur key frames with 255, 256, 257 and 300 key lines, neighbours with 70 and with 300, groups of three pairs (RGB-D)
    -> (scene, groups, matches)"""
    if "counts" not in _wide:
        scene = make_scene(70, KP.RGBD, F=10, n_seg=640, n_long=4, cap=WIDE_CAP, counts=(255, 70, 256, 300, 257, 70, 300, 300, 300, 0))
        assert [len(kf["keylines"]) for kf in scene["kfs"]] == [255, 70, 256, 300, 257, 70, 300, 300, 300, 0]
        groups = [(0, [1, 3, 6]), (2, [3, 5, 7]), (4, [5, 6, 1]), (6, [7, 1, 3])]
        _wide["counts"] = (scene, groups, match_all(scene, groups))
    return _wide["counts"]


SHARED_QUERIES, SHARED_TRAIN = (10, 266, 290), (260, 280)        # three query slots on both sides of 256, the train index per neighbour
SHARED_CASES = ("free", "cur occupied", "train occupied")


def shared_train_case():
    """L2: one group (0, [2, 4]) of full key frames (monocular, nothing occupied); query slots SHARED_QUERIES of key frame 0 are copies of one
    key line whose partner is slot SHARED_TRAIN[k] of neighbour k -> (scene, groups, matches, occupancy per case of SHARED_CASES)"""
    if "shared" not in _wide:
        scene = make_scene(71, KP.MONOCULAR, F=7, n_seg=640, cap=WIDE_CAP, counts=(WIDE_CAP,) * 6 + (0,), occupied_rate=0.0)
        groups = [(0, [2, 4])]
        assert all(len(scene["kfs"][k]["keylines"]) == WIDE_CAP for k in (0, 2, 4))
        matches = [plant_shared_train(scene, 0, groups[0][1], SHARED_QUERIES, SHARED_TRAIN)]
        free = [np.zeros(len(kf["keylines"]), np.uint8) for kf in scene["kfs"]]
        occ = {"free": free, "cur occupied": [o.copy() for o in free], "train occupied": [o.copy() for o in free]}
        occ["cur occupied"][0][SHARED_QUERIES[0]] = 1
        occ["train occupied"][2][SHARED_TRAIN[0]] = 1
        _wide["shared"] = (scene, groups, matches, occ)
    return _wide["shared"]


KP_COUNT = 260


def kp_depth_case():
    """L3: stereo; key frame 0 has WIDE_CAP key lines and KP_COUNT key points, its neighbours have more key points than key lines
    -> (scene, groups, matches)"""
    if "kp" not in _wide:
        scene = make_scene(72, KP.STEREO, F=7, n_seg=640, cap=WIDE_CAP, counts=(WIDE_CAP, 250, 250, 250, 250, 250, 0), few_keypoints=False,
                           n_keypoints={0: KP_COUNT})
        assert len(scene["kfs"][0]["keylines"]) == WIDE_CAP and len(scene["kfs"][0]["kp_depths"]) == KP_COUNT
        groups = [(0, [2, 4, 1])]
        _wide["kp"] = (scene, groups, match_all(scene, groups))
    return _wide["kp"]


def limit_case():
    """L4: cap = LIMIT_CAP; a small monocular scene whose key frames 0 and 2 are repeated up to the capacity, one group (0, [2, 4]).  The
    small scene's 1-NN for its own slots, no match (the distance gate) for the repeated ones; planted: query LIMIT_CAP - 1 (a copy of a
    query that is created) and train index 8100 (a copy of the partner of another) -> (scene, groups, matches, planted)"""
    if "limit" not in _wide:
        scene = make_scene(73, KP.MONOCULAR, F=7, occupied_rate=0.0)
        groups = [(0, [2, 4])]
        base = match_all(scene, groups)[0]
        nb = len(scene["kfs"][0]["keylines"])
        made = [(j, int(base[0][0][j])) for j in range(nb) if base[0][0][j] >= 0 and created_alone(scene, 0, 2, j, int(base[0][0][j]), dist=base[0][1][j])]
        made = [(j, t) for j, t in made if [tt for _, tt in made].count(t) == 1]
        (j1, t1), (j2, t2) = made[0], made[1]
        tile_key_frame(scene, 0, LIMIT_CAP)
        tile_key_frame(scene, 2, LIMIT_CAP)
        last, far = LIMIT_CAP - 1, 8100
        copy_slot(scene, 0, j1, last)
        copy_slot(scene, 2, t2, far)
        matches = []
        for ti, di in base:
            a, b = np.full(LIMIT_CAP, -1, np.int32), np.full(LIMIT_CAP, 256, np.int32)
            a[:nb], b[:nb] = ti, di
            matches.append((a, b))
        ti, di = matches[0]
        ti[last], di[last] = t1, di[j1]
        ti[j1], di[j1] = -1, 256                                # its copy at the last slot takes its place
        ti[j2] = far
        _wide["limit"] = (scene, groups, [matches], dict(created=[(0, last, t1), (0, j2, far)]))
    return _wide["limit"]


def wide_reference(case, gates_name="mapping", occupancy=None):
    """the restatement on a wide case, once per process -> dict(ref = (match, pos_w, status, occupied_cur), gaps, info)"""
    key = ("ref", case, gates_name, occupancy)
    if key not in _wide:
        gates = dict(mapping=KP.MAPPING_GATES, unchecked=NO_GATES_CHECK)[gates_name]
        gaps, info = [], []
        if case == "counts":
            scene, groups, matches = wide_counts_case()
            ref = run_ref(scene, groups, matches, gates, gaps, info, cap=WIDE_CAP)
        elif case == "shared":
            scene, groups, matches, occ = shared_train_case()
            ref = run_ref(scene, groups, matches, gates, gaps, info, occupied=occ[occupancy], cap=WIDE_CAP)
        elif case == "kp":
            scene, groups, matches = kp_depth_case()
            ref = run_ref(scene, groups, matches, gates, gaps, info, cap=WIDE_CAP)
        else:
            scene, groups, matches, _ = limit_case()
            ref = run_ref(scene, groups, matches, gates, gaps, info, cap=LIMIT_CAP)
        _wide[key] = dict(ref=ref, gaps=gaps, info=info)
    return _wide[key]
