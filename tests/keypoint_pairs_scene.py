"""Synthetic scenes with ground truth for the key-frame pair point triangulation tests (CPU and GPU use the same inputs, so what the CPU
tests assert about the restatement's output -- every status reached, no near tie in a comparison that depends on the null vector or on a
libm result -- holds for the GPU comparison).

A scene: random 3-D points in front of a rig of key frames with real poses, projected with the camera model's restatement, perturbed by a
fraction of a pixel, slots shuffled per key frame, ragged counts.  Key frame 0 has the identity pose; key frame 2 stands 16 cm in front of
it (little parallax: NO_PARALLAX, and the stereo branches of a stereo / RGB-D setup); key frame 3 is one centimetre from key frame 1 (the
baseline gate skips the pair); key frame F - 2 stands behind the rig (as kf1 of a pair its centre has z <= 0 in kf2: the un-normalised
epipole); key frame F - 1 is empty.  Matches come from the ground truth: most key points of kf2 that see a point kf1 sees too are matched
with it, some with another key point (wrong pairings for the depth, reprojection and scale checks); the query slots are a permutation of
kf1's key points, as the BoW node order of the matcher's queries is; planted slots reach INDEX_RANGE and NON_FINITE."""
import functools
import importlib
import math

import numpy as np

import keypoint_pairs_ref as KR
from landmark_observe_ref import frame_pose, reproject, scale_factors

plp = importlib.import_module("structure-plp-slam_amd")
f32, f64 = np.float32, np.float64
CAMS = dict(
    perspective=dict(model="perspective", cols=640, rows=480, fx=500.0, fy=500.0, cx=320.0, cy=240.0, focal_x_baseline=50.0),
    fisheye=dict(model="fisheye", cols=640, rows=480, fx=380.0, fy=382.0, cx=318.5, cy=241.25, focal_x_baseline=38.0),
    equirectangular=dict(model="equirectangular", cols=1920, rows=960, fx=0.0, fy=0.0, cx=0.0, cy=0.0, focal_x_baseline=0.0))
TRUE_BASELINE = 0.1
NUM_LEVELS, SCALE_FACTOR = 8, 1.2
CAP = 80                                                        # not a multiple of 64
SENT_I32, SENT_U8, SENT_F64 = -77, 0xEE, -12345.5
SETUPS = [(KR.MONOCULAR, "perspective"), (KR.MONOCULAR, "fisheye"), (KR.MONOCULAR, "equirectangular"), (KR.RGBD, "perspective"),
          (KR.RGBD, "fisheye"), (KR.STEREO, "perspective"), (KR.STEREO, "fisheye")]


def scale_tables():
    sf = scale_factors(SCALE_FACTOR, NUM_LEVELS)
    return sf, (sf * sf).astype(np.float32)                     # level_sigma_sq_ = scale_factors_^2 (orb_params::calc_level_sigma_sq)


def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _poses(rng, F):
    out = []
    for k in range(F):
        if k == 0:
            R, c = np.eye(3), np.zeros(3)
        elif k == 2:
            R, c = _rot(rng.normal(size=3) * 0.002), np.array([0.02, 0.01, 0.16])
        elif k == 3:
            R, c = out[1][0] @ _rot(rng.normal(size=3) * 0.001), out[1][1] + np.array([0.006, -0.005, 0.006])
        elif k == F - 2:
            R, c = _rot(rng.normal(size=3) * 0.02), np.array([0.15, 0.05, -0.9])
        else:
            R, c = _rot(rng.normal(size=3) * 0.05), rng.uniform(-0.8, 0.8, 3) * np.array([1.0, 0.5, 0.4])
        out.append((R, c))
    return out


def _observe(cam, P, X, noise, rng):
    """-> (pt f32 (2,), bearing f64 (3,), depth z) of the point seen with a perturbation of about `noise` pixels, or None when not visible"""
    Xc = np.array([P[0:3] @ X + P[9], P[3:6] @ X + P[10], P[6:9] @ X + P[11]])
    if cam["model"] == "equirectangular":
        d = Xc / np.linalg.norm(Xc) + rng.normal(size=3) * noise * (2 * math.pi / cam["cols"])
        d /= np.linalg.norm(d)
        lon, lat = math.atan2(d[0], d[2]), -math.asin(d[1])
        pt = np.array([cam["cols"] * (0.5 + lon / (2 * math.pi)), cam["rows"] * (0.5 - lat / math.pi)], np.float32)
        return pt, d, Xc[2]
    if Xc[2] <= 0.3:
        return None
    u = cam["fx"] * Xc[0] / Xc[2] + cam["cx"] + rng.normal() * noise
    v = cam["fy"] * Xc[1] / Xc[2] + cam["cy"] + rng.normal() * noise
    if not (0 < u < cam["cols"] and 0 < v < cam["rows"]):
        return None
    pt = np.array([u, v], np.float32)
    b = np.array([(f64(pt[0]) - cam["cx"]) / cam["fx"], (f64(pt[1]) - cam["cy"]) / cam["fy"], 1.0])
    return pt, b / np.linalg.norm(b), Xc[2]


def make_scene(seed, setup_type, model, F=9, n_pts=70, noise=0.25, cap=CAP, counts=None, drop=0.12, wrong_octave=0.08):
    """-> dict(cam, setup_type, F, kfs: the restatement's key-frame dicts (+ pid: the point of every slot, median_depth), points).
    cap: the slots of the table the scene is made for; counts: per key frame the ragged cut (None: cap - 6, - 11, - 16 in turn), so that a
    key frame can fill the capacity; drop / wrong_octave: the share of points a key frame misses / sees at a random octave."""
    rng = np.random.default_rng(seed)
    cam = CAMS[model]
    pts = np.stack([rng.uniform(-2.2, 2.2, n_pts), rng.uniform(-1.6, 1.6, n_pts), rng.uniform(3.0, 9.0, n_pts)], 1)
    kfs = []
    for k, (R, c) in enumerate(_poses(rng, F)):
        P = frame_pose(R, -R @ c)
        rows = []
        if k != F - 1:
            for i in rng.permutation(n_pts):
                if rng.uniform() < drop:
                    continue
                o = _observe(cam, P, pts[i], noise, rng)
                if o is None:
                    continue
                pt, b, z = o
                dist = np.linalg.norm(pts[i] - c)
                octave = int(np.clip(round(math.log(dist / 3.0) / math.log(SCALE_FACTOR)), 0, NUM_LEVELS - 1))
                if rng.uniform() < wrong_octave:
                    octave = int(rng.integers(0, NUM_LEVELS))   # a wrong octave: the scale check, the thresholds
                xr, depth = f32(-1.0), f32(-1.0)
                if setup_type != KR.MONOCULAR and rng.uniform() < 0.7:
                    depth = f32(z * (1 + rng.normal() * 2e-3))
                    xr = f32(f64(pt[0]) - cam["focal_x_baseline"] / f64(depth))
                    if rng.uniform() < 0.04:
                        depth = f32(0.0)                        # stereo without a depth: triangulate_stereo returns the zero vector
                rows.append((pt, b, xr, depth, octave, int(i)))
        rows = rows[:cap - 6 - (k % 3) * 5 if counts is None else min(int(counts[k]), cap)]   # ragged
        n = len(rows)
        kp = np.zeros(n, plp.KP_DTYPE)
        kp["x"], kp["y"] = [r[0][0] for r in rows], [r[0][1] for r in rows]
        kp["octave"], kp["size"], kp["class_id"] = [r[4] for r in rows], 31.0, -1
        kp["angle"] = rng.uniform(0, 360, n)
        kf = dict(keypts=kp, bearings=np.array([r[1] for r in rows], np.float64).reshape(n, 3), x_right=np.array([r[2] for r in rows], np.float32),
                  depths=np.array([r[3] for r in rows], np.float32), pose=P, pid=np.array([r[5] for r in rows], np.int64))
        zs = np.sort(np.array([abs(P[6:9] @ pts[i] + P[11]) for i in kf["pid"]], np.float32))
        kf["median_depth"] = zs[(n - 1) // 2] if n else f32(0.0)
        kfs.append(kf)
    # planted: a key point at infinity (its reprojection error is not finite), an octave outside the table (clamped)
    if F > 6 and len(kfs[4]["keypts"]) > 3:
        kfs[4]["keypts"]["x"][1] = np.inf
        kfs[4]["x_right"][1], kfs[4]["depths"][1] = -1.0, -1.0
        kfs[5]["keypts"]["octave"][2] = 11
        kfs[6]["keypts"]["octave"][0] = -3
    return dict(cam=cam, setup_type=setup_type, model=model, F=F, kfs=kfs, points=pts)


def default_pairs(scene):
    """(kf1 = cur, kf2 = ngh): ordinary pairs, the little-parallax pair both ways, the gated pair, the key frame behind the rig as kf1 and
    as kf2, an empty key frame on either side"""
    F = scene["F"]
    return np.array([(0, 1), (1, 4), (4, 5), (5, 0), (0, 2), (2, 0), (1, 3), (F - 2, 0), (0, F - 2), (4, 6), (6, 1), (F - 1, 0), (1, F - 1),
                     (5, 4), (6, 5)], np.int32)


def make_matches(scene, pairs, seed, wrong=0.14, drop=0.12, cap=CAP):
    """ground-truth matches in the matcher's layout -> (match_q (P, cap) i32, q_feature (P, cap) i32); slots past a key frame's count hold 0"""
    rng = np.random.default_rng(seed)
    Pn = len(pairs)
    mq, qf = np.zeros((Pn, cap), np.int32), np.zeros((Pn, cap), np.int32)
    for p, (f1, f2) in enumerate(pairs):
        k1, k2 = scene["kfs"][f1], scene["kfs"][f2]
        n1, n2 = len(k1["keypts"]), len(k2["keypts"])
        order = rng.permutation(n1)                             # query slot -> key point of kf1
        qf[p, :n1] = order
        qf[p, n1:] = n1 + 3                                     # unused query slots name a key point that does not exist
        slot_of = {int(j): q for q, j in enumerate(order)}
        by_pid = {int(pid): j for j, pid in enumerate(k1["pid"])}
        used = set()
        mq[p, :n2] = -1
        for t in range(n2):
            j = by_pid.get(int(k2["pid"][t]))
            if n1 and rng.uniform() < wrong:
                j = int(rng.integers(0, n1))
            if j is None or rng.uniform() < drop or j in used:
                continue
            used.add(j)
            mq[p, t] = slot_of[j]
        if n2 > 4 and n1 < cap:
            mq[p, n2 - 1] = n1                                  # planted: a query slot whose key point is outside kf1 (INDEX_RANGE)
            mq[p, n2 - 2] = cap + 5                             # planted: a query slot outside [0, m_cap) (NO_MATCH)
    return mq, qf


def table(scene, cap=CAP):
    """the key-frame table as plp_triangulate_keypoint_pairs_* takes it: arrays with leading dimension F, cap slots"""
    F = scene["F"]
    t = dict(keypts=np.zeros((F, cap), plp.KP_DTYPE), bearings=np.zeros((F, cap, 3), np.float64), x_right=np.full((F, cap), -1, np.float32),
             depths=np.full((F, cap), -1, np.float32), counts=np.zeros(F, np.int32), pose=np.zeros((F, 15), np.float64),
             median_depth=np.zeros(F, np.float32))
    for k, kf in enumerate(scene["kfs"]):
        n = len(kf["keypts"])
        t["keypts"][k, :n], t["bearings"][k, :n], t["x_right"][k, :n], t["depths"][k, :n] = kf["keypts"], kf["bearings"], kf["x_right"], kf["depths"]
        t["counts"][k], t["pose"][k], t["median_depth"][k] = n, kf["pose"], kf["median_depth"]
    return t


def reference_geometry(scene, pairs):
    """-> (skip (P,) u8, epipolar (P, 12) f64, baseline (P,) f64) of the restatement"""
    Pn = len(pairs)
    skip, epi, base = np.zeros(Pn, np.uint8), np.zeros((Pn, 12), np.float64), np.zeros(Pn, np.float64)
    for p, (f1, f2) in enumerate(pairs):
        k1, k2 = scene["kfs"][f1], scene["kfs"][f2]
        s, e, b = KR.pair_geometry(scene["cam"], scene["setup_type"], TRUE_BASELINE, k1["pose"], k2["pose"], k2["median_depth"])
        skip[p], epi[p], base[p] = s, e, b
    return skip, epi, base


def reference_pairs(scene, pairs, mq, qf, pair_skip=None, occ1=None, occ2=None, null=KR.null_vector4, gaps=None, infos=None, cap=CAP):
    """the restatement over all pairs -> (idx_1 (P, cap) i32, pos_w (P, cap, 3), status (P, cap) u8, occ1, occ2 (P, cap) u8), every slot the
    library does not write holding its sentinel (occ1 / occ2: the given arrays, updated where a landmark is created)"""
    sf, ls = scale_tables()
    Pn = len(pairs)
    idx = np.full((Pn, cap), SENT_I32, np.int32); pos = np.full((Pn, cap, 3), SENT_F64, np.float64); st = np.full((Pn, cap), SENT_U8, np.uint8)
    o1 = None if occ1 is None else occ1.copy()
    o2 = None if occ2 is None else occ2.copy()
    for p, (f1, f2) in enumerate(pairs):
        k1, k2 = scene["kfs"][f1], scene["kfs"][f2]
        n2 = len(k2["keypts"])
        sk = bool(pair_skip is not None and pair_skip[p])
        info = [] if infos is not None else None
        i, x, s = KR.triangulate_pair(scene["cam"], scene["setup_type"], TRUE_BASELINE, sf, ls, SCALE_FACTOR, 1.0, k1, k2, mq[p],
                                      None if qf is None else qf[p], cap if qf is None else qf.shape[1], sk,
                                      None if o1 is None else o1[p], None if o2 is None else o2[p], null, gaps, info)
        st[p, :n2] = s
        if not sk:
            idx[p, :n2], pos[p, :n2] = i, x
        if infos is not None:
            infos.append(info)
    return idx, pos, st, o1, o2


def add_descriptors(scene, seed, nodes=12, flips=6):
    """ORB-like descriptors and BoW nodes for the matcher: a 256-bit code per 3-D point with a few bits flipped per view; the node is a
    function of the point (a few views fall into another node, as quantisation does).  Adds desc (n, 32) u8 and node (n,) i32 per key frame."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (len(scene["points"]), 32), dtype=np.uint8)
    for kf in scene["kfs"]:
        n = len(kf["keypts"])
        d = codes[kf["pid"]].copy().reshape(n, 32)
        for j in range(n):
            for _ in range(int(rng.integers(0, flips))):
                d[j, rng.integers(0, 32)] ^= np.uint8(1 << int(rng.integers(0, 8)))
        node = (kf["pid"] * 7 + 3) % nodes
        stray = rng.uniform(size=n) < 0.05
        node[stray] = rng.integers(0, nodes, int(stray.sum()))
        kf["desc"], kf["node"] = d, node.astype(np.int32)
    return scene


# ------------------------------------------------------------------------------------------ above one workgroup of slots (256 of key frame 2)
# The scenes of tests/test_gpu_pair_kernels_wide.py; what they are named for is asserted on the restatement in tests/test_pair_kernels_wide_cpu.py.
WIDE_CAP = 520                                                  # three workgroups, the last with 8 slots; not a multiple of 64
WIDE_COUNTS = (255, 256, 257, 511, 512, 513)                    # key frame 2's counts around one and two workgroups
WIDE_SETUPS = [(KR.RGBD, "perspective"), (KR.MONOCULAR, "fisheye"), (KR.MONOCULAR, "equirectangular")]   # one per camera template
LIMIT_CAP = 8192                                                # the largest capacity the entries accept
_SLOT_FIELDS = ("keypts", "bearings", "x_right", "depths", "pid")


def swap_slots(kf, a, b):
    """exchange two key points of a key frame (every per-slot array)"""
    for k in _SLOT_FIELDS:
        kf[k][[a, b]] = kf[k][[b, a]]


def planted_matches(scene, pairs, slots, seed, cap=CAP, permute=True):
    """matches planted by slot -> (match_q (P, cap), q_feature (P, cap)): slots[p] lists the slots of key frame 2 that are matched in pair p,
    each an int t (its partner: the key point of key frame 1 that sees the same point; where there is none or it is taken, the first key
    point that is free -- a wrong pairing, still a match) or (t, j) with the key point j of key frame 1 named (j outside key frame 1 is
    given a query slot of its own behind the permutation: INDEX_RANGE).  Every other slot below the count holds -1.  permute: the query
    slots are a permutation of key frame 1's key points, as in make_matches; otherwise query slot = key point."""
    rng = np.random.default_rng(seed)
    Pn = len(pairs)
    mq, qf = np.zeros((Pn, cap), np.int32), np.zeros((Pn, cap), np.int32)
    for p, (f1, f2) in enumerate(pairs):
        k1, k2 = scene["kfs"][f1], scene["kfs"][f2]
        n1, n2 = len(k1["keypts"]), len(k2["keypts"])
        order = rng.permutation(n1) if permute else np.arange(n1)
        qf[p, :n1], qf[p, n1:] = order, n1 + 3
        slot_of = {int(j): q for q, j in enumerate(order)}
        by_pid = {int(pid): j for j, pid in enumerate(k1["pid"])}
        mq[p, :n2] = -1
        named = [e for e in slots[p] if not isinstance(e, (int, np.integer))]
        used, spare, free = {int(j) for _, j in named}, n1, 0
        for t, j in named:
            if 0 <= j < n1:
                mq[p, t] = slot_of[int(j)]
            else:
                assert spare < cap, "no query slot left behind key frame 1's"
                qf[p, spare], mq[p, t] = j, spare
                spare += 1
        for t in (e for e in slots[p] if isinstance(e, (int, np.integer))):
            assert 0 <= t < n2 and mq[p, t] == -1, (p, t)
            j = by_pid.get(int(k2["pid"][t]))
            if j is None or j in used:
                while free in used:
                    free += 1
                j = free
            assert j < n1, "more matches than key frame 1 has key points"
            used.add(j)
            mq[p, t] = slot_of[j]
    return mq, qf


def direct_matches(scene, pairs, mq, qf):
    """the same matches for q_feature = NULL: the key-point index in place of the query slot (what is no key point of the table: -1)"""
    cap = mq.shape[1]
    direct = np.full_like(mq, -1)
    for p in range(len(pairs)):
        n2 = len(scene["kfs"][pairs[p][1]]["keypts"])
        for t in range(n2):
            direct[p, t] = qf[p, mq[p, t]] if 0 <= mq[p, t] < qf.shape[1] else -1
        direct[p, n2:] = mq[p, n2:]
    assert cap == qf.shape[1]
    return direct


def _status_of(scene, f1, f2, j, t):
    sf, ls = scale_tables()
    return KR.triangulate(scene["cam"], scene["setup_type"], TRUE_BASELINE, sf, ls, SCALE_FACTOR, KR.cos_parallax_thr(1.0), scene["kfs"][f1],
                          scene["kfs"][f2], j, t)[0]


def place_created_pair(scene, f1, f2, j_to, t_to, keep1=(), keep2=()):
    """move a ground-truth pair that the restatement turns into a landmark to key point j_to of key frame f1 and slot t_to of key frame f2
    (by exchanging slots inside each key frame; the slots in keep1 / keep2 are left alone)"""
    k1, k2 = scene["kfs"][f1], scene["kfs"][f2]
    by_pid = {int(pid): j for j, pid in enumerate(k1["pid"])}
    for t in range(len(k2["keypts"])):
        j = by_pid.get(int(k2["pid"][t]))
        if j is None or j in keep1 or t in keep2 or _status_of(scene, f1, f2, j, t) != KR.CREATED:
            continue
        swap_slots(k1, j, j_to)
        swap_slots(k2, t, t_to)
        return
    raise AssertionError("no ground-truth pair of this scene is created")


@functools.lru_cache(maxsize=None)
def wide_counts_case(wi):
    """K1: key frame 0 with WIDE_CAP key points against six neighbours with WIDE_COUNTS; dense ground-truth matches; NON_FINITE, INDEX_RANGE,
    NO_MATCH and octaves outside the table planted at slots at or above 256 -> (scene, pairs, match_q, q_feature)"""
    setup, model = WIDE_SETUPS[wi]
    counts = (WIDE_CAP,) + WIDE_COUNTS + (0,)
    sc = make_scene(400 + wi, setup, model, F=8, n_pts=1100, cap=WIDE_CAP, counts=counts)
    assert tuple(len(kf["keypts"]) for kf in sc["kfs"]) == counts
    for f, t in ((4, 256), (5, 300), (5, 301), (5, 419), (6, 257), (6, 300)):   # a key point at infinity: its reprojection error is not finite
        sc["kfs"][f]["keypts"]["x"][t] = np.inf
        sc["kfs"][f]["x_right"][t], sc["kfs"][f]["depths"][t] = -1.0, -1.0
    sc["kfs"][4]["keypts"]["octave"][260], sc["kfs"][4]["keypts"]["octave"][300] = 11, -3
    # the one slot of the second workgroup (n2 = 257) and of the third (513) become landmarks, with the last key points of key frame 1
    place_created_pair(sc, 0, 3, WIDE_CAP - 2, 256)
    place_created_pair(sc, 0, 6, WIDE_CAP - 1, 512, keep1=(WIDE_CAP - 2,))
    pairs = np.array([(0, k) for k in range(1, 7)], np.int32)
    mq, qf = make_matches(sc, pairs, 500 + wi, cap=WIDE_CAP)
    for p, t, j in ((2, 256, WIDE_CAP - 2), (5, 512, WIDE_CAP - 1)):
        q = int(np.nonzero(qf[p] == j)[0][0])
        mq[p, :t][mq[p, :t] == q] = -1
        mq[p, t] = q
    for p in range(len(pairs)):                                 # key frame 1 fills the capacity: make_matches plants nothing
        live = [t for t in range(256, min(counts[1 + p], 512)) if mq[p, t] >= 0]
        if len(live) >= 3:
            qf[p, mq[p, live[-1]]] = WIDE_CAP                   # a key point outside key frame 1 (INDEX_RANGE), in the second workgroup
            qf[p, mq[p, live[-2]]] = -2
            mq[p, live[-3]] = WIDE_CAP + 5                      # a query slot outside [0, m_cap) (NO_MATCH)
    return sc, pairs, mq, qf


WIDE_LAYOUTS = [
    ("workgroup 0 full, workgroup 1 empty", list(range(0, 256))),
    ("last wave only", list(range(192, 256)) + list(range(448, 512))),
    ("lane 0 of every wave", list(range(0, WIDE_CAP, 64))),
    ("lane 63 of every wave", list(range(63, WIDE_CAP, 64))),
    ("slots 255, 256, 519", [255, 256, 519]),
    ("no match", []),
]


@functools.lru_cache(maxsize=None)
def wide_layout_case():
    """K2 / K4: two key frames that fill WIDE_CAP, every point seen by both at its own octave; one pair per layout of WIDE_LAYOUTS, then the
    pair once more with dense matches twice (K4 skips the first of the two) -> (scene, pairs, match_q, q_feature, pair_skip)"""
    sc = make_scene(450, KR.MONOCULAR, "perspective", F=4, n_pts=900, cap=900, counts=(900, 900, 0, 0), drop=0.0, wrong_octave=0.0)
    both = np.intersect1d(sc["kfs"][0]["pid"], sc["kfs"][1]["pid"])[:WIDE_CAP]
    for kf in sc["kfs"][:2]:                                    # the same WIDE_CAP points in both key frames, each in its own slot order
        rows = np.isin(kf["pid"], both)
        for k in _SLOT_FIELDS:
            kf[k] = kf[k][rows]
    assert [len(kf["keypts"]) for kf in sc["kfs"]] == [WIDE_CAP, WIDE_CAP, 0, 0]
    n = len(WIDE_LAYOUTS)
    pairs = np.array([(0, 1)] * (n + 2), np.int32)
    dense = list(range(WIDE_CAP))
    mq, qf = planted_matches(sc, pairs, [s for _, s in WIDE_LAYOUTS] + [dense, dense], 451, cap=WIDE_CAP)
    skip = np.zeros(n + 2, np.uint8)
    skip[n] = 1
    return sc, pairs, mq, qf, skip


@functools.lru_cache(maxsize=None)
def limit_case():
    """K3: cap = m_cap = LIMIT_CAP, key frame 0 with 8000 key points, key frame 1 full, key frame 2 empty; a few hundred planted matches, the
    last slot with the last key point, INDEX_RANGE at key point 8000, NO_MATCH at query m_cap -> (scene, pairs, match_q, q_feature, planted)"""
    n1 = 8000
    sc = make_scene(460, KR.MONOCULAR, "perspective", F=3, n_pts=15000, cap=LIMIT_CAP, counts=(n1, LIMIT_CAP, 0))
    assert [len(kf["keypts"]) for kf in sc["kfs"]] == [n1, LIMIT_CAP, 0]
    place_created_pair(sc, 0, 1, n1 - 1, LIMIT_CAP - 1)
    place_created_pair(sc, 0, 1, n1 - 2, 0, keep1=(n1 - 1,), keep2=(LIMIT_CAP - 1,))
    pairs = np.array([(0, 1), (0, 2), (1, 0)], np.int32)
    first = [t for t in range(27, LIMIT_CAP - 3, 27)] + [(LIMIT_CAP - 1, n1 - 1), (0, n1 - 2), (LIMIT_CAP - 2, n1)]
    back = [t for t in range(5, n1 - 1, 61)] + [n1 - 1]
    mq, qf = planted_matches(sc, pairs, [first, [], back], 461, cap=LIMIT_CAP)
    mq[0, LIMIT_CAP - 3] = LIMIT_CAP                            # a query slot at m_cap
    planted = dict(created=[(0, LIMIT_CAP - 1, n1 - 1), (0, 0, n1 - 2)], index_range=[(0, LIMIT_CAP - 2, n1)], no_match=[(0, LIMIT_CAP - 3)])
    return sc, pairs, mq, qf, planted


@functools.lru_cache(maxsize=None)
def wide_reference(case, *args):
    """the restatement on a wide case, once per process -> dict(ref = (idx_1, pos_w, status, None, None), gaps, infos); the caller's occupancy
    is applied by the test (expect_occupancy).  case: "counts" (wi, permuted), "layout", "limit"."""
    gaps, infos = [], []
    if case == "counts":
        wi, permuted = args
        sc, pairs, mq, qf = wide_counts_case(wi)
        if not permuted:
            mq, qf = direct_matches(sc, pairs, mq, qf), None
        ref = reference_pairs(sc, pairs, mq, qf, None, gaps=gaps, infos=infos, cap=WIDE_CAP)
    elif case == "layout":
        sc, pairs, mq, qf, skip = wide_layout_case()
        ref = reference_pairs(sc, pairs, mq, qf, skip, gaps=gaps, infos=infos, cap=WIDE_CAP)
    else:
        sc, pairs, mq, qf, _ = limit_case()
        ref = reference_pairs(sc, pairs, mq, qf, None, gaps=gaps, infos=infos, cap=LIMIT_CAP)
    return dict(ref=ref, gaps=gaps, infos=infos)
