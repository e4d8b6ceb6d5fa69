"""Seeded map snapshots for the map-culling tests, small enough for an object-level restatement yet at the sizes the
kernels of csrc/map_cull_kernels.hip can go wrong at: key frames of 63, 64, 65 and 257 key points (the wave, and one past the workgroup of 256),
observation lists of 0, 1, 3, 4 and more than 64 entries, covisibility lists of 0, 1 and more than 64 entries, F = 65 and 97 (the removed set's
bitmap words), monocular, stereo and RGB-D tables.

A scene is a random base map plus key frames steered to the cases the census of tests/test_map_cull_cpu.py asks for.  The steered key frames sit
in rows of their own whose slots hold designed landmarks only, so their counts are exact:

  redundant landmark of K   K at octave 6, four helpers at octave 0 (and, first in the list, one at octave 9 that is no better): num_observations
                            above 3, three better observers, the third of them the list's last entry for the first such landmark
  plain landmark of K       K and one helper: valid, never redundant
  Z                         removed early: redundant landmarks, plus base landmarks it sees at octave 7
  FLIP_RK                   ten landmarks whose third better observer is Z: the snapshot says 10 / 10, after Z's removal 0 / 10
  FLIP_KR                   nine redundant landmarks and two seen by Z and one helper only, which the cascade discards: 9 / 11, then 9 / 9
"""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
ORIGIN_ID, CUR_ID = 7, 1000
STEERED = ("CUR", "CUR2", "ORIGIN", "W_AT", "W_M2", "W_M3", "W_P1", "EMPTY", "K910", "K89", "HELD", "ERASED", "Z", "FLIP_RK", "FLIP_KR",
           "H0", "H1", "H2", "H3", "H5")


class Builder:
    def __init__(self, F, cap, setup, seed):
        self.rng = np.random.default_rng(seed)
        self.F, self.cap, self.setup = F, cap, setup                  # setup 0 monocular, 1 stereo, 2 RGB-D
        self.kf_lm = np.full((F, cap), -1, np.int32)
        self.undist = np.zeros((F, cap), KP_DTYPE)
        self.undist["octave"] = self.rng.integers(0, 8, (F, cap))
        self.x_right = np.full((F, cap), -1.0, np.float32)
        self.depths = self.rng.uniform(0.5, 30.0, (F, cap)).astype(np.float32)
        self.depth_thr = np.full(F, 40.0, np.float32)
        self.counts = np.zeros(F, np.int32)
        self.free = [[] for _ in range(F)]
        self.obs = []                                                 # per landmark: [(kf, idx)]
        self.name = {n: F - 1 - i for i, n in enumerate(STEERED)}     # the steered rows are the last ones
        self.base = F - len(STEERED)

    def slots(self, kf, n):
        """key frame kf has n key points, handed out in a random order"""
        self.counts[kf] = n
        self.free[kf] = [int(v) for v in self.rng.permutation(n)]

    def observe(self, lm, kf, octave=None, stereo=None):
        if not self.free[kf]:
            return False
        idx = self.free[kf].pop()
        self.kf_lm[kf, idx] = lm
        if octave is not None:
            self.undist["octave"][kf, idx] = octave
        if self.setup:                                                # stereo: some key points have no right match; RGB-D: all have one
            has = bool(self.rng.integers(0, 4)) if stereo is None else stereo
            self.x_right[kf, idx] = np.float32(self.rng.uniform(0, 600)) if (has or self.setup == 2) else np.float32(-1.0)
        self.obs[lm].append((kf, idx))
        return True

    def landmark(self, observers):
        """a landmark seen by (kf name or row, octave) in list order; its row"""
        lm = len(self.obs)
        self.obs.append([])
        for kf, octave in observers:
            self.observe(lm, self.name.get(kf, kf), octave)
        return lm

    def redundant(self, k, n, first_last=False):
        for i in range(n):
            self.landmark([(k, 6), ("H5", 9), ("H0", 0), ("H1", 0), ("H2", 0)] if first_last and i == 0 else
                          [(k, 6), ("H0", 0), ("H1", 0), ("H2", 0), ("H3", 0)])

    def plain(self, k, n):
        for _ in range(n):
            self.landmark([(k, 3), ("H0", 0)])


def keyframe_scene(F, setup, seed, problems, lm_num_obs=False, outside=False, wrap=False):
    cap = 260
    b = Builder(F, cap, setup, seed)
    rng = b.rng
    sizes = [63, 64, 65, 257]
    for f in range(b.base):
        b.slots(f, sizes[f] if f < len(sizes) else int(rng.integers(70, 200)))
    for n in STEERED:
        b.slots(b.name[n], cap)
    # the base map: lists of every length the kernels' loops treat apart, one of them through every base key frame
    lengths = [0, 1, 3, 4, b.base] + [int(v) for v in rng.choice([2, 3, 4, 5, 6, 8, 12], 40 * b.base)]
    for n in lengths:
        if not any(b.free[f] for f in range(b.base)):
            break
        b.landmark([(int(f), None) for f in rng.permutation(b.base)[:n]])
    n_base = len(b.obs)
    # the steered key frames
    b.redundant("K910", 9, first_last=True); b.plain("K910", 1)
    b.redundant("K89", 8); b.plain("K89", 1)
    b.redundant("HELD", 10)
    b.redundant("W_M3", 2); b.plain("W_M3", 3)
    b.redundant("W_P1", 1); b.plain("W_P1", 4)
    b.redundant("W_AT", 10); b.redundant("W_M2", 10); b.redundant("ORIGIN", 10)          # removable, were they not skipped
    b.redundant("Z", 5)
    seen = 0
    for lm in range(n_base):                                                              # a hundred base landmarks Z sees as redundant
        if len(b.obs[lm]) >= 4 and rng.integers(0, 3) == 0 and seen < 100:
            seen += b.observe(lm, b.name["Z"], 7)
    for _ in range(10):
        b.landmark([("H5", 9), ("H0", 0), ("H1", 0), ("FLIP_RK", 6), ("Z", 7)])
    b.redundant("FLIP_KR", 9)
    for _ in range(2):
        b.landmark([("FLIP_KR", 3), ("Z", 3), ("H0", 0)])
    L = len(b.obs)
    # ERASED: erased before the call, so no list names it, but its landmarks_ still hold what was not discarded (keyframe.cc:892-899)
    e = b.name["ERASED"]
    for i in range(10):
        lm = b.landmark([("H0", 0), ("H1", 0), ("H2", 0), ("H3", 0)])
        b.kf_lm[e, b.free[e].pop()] = lm
    L = len(b.obs)
    kf_id = (10 + 3 * np.arange(F)).astype(np.uint32)
    for n, v in (("CUR", CUR_ID), ("CUR2", 2000), ("ORIGIN", ORIGIN_ID), ("W_AT", CUR_ID), ("W_M2", CUR_ID - 2), ("W_M3", CUR_ID - 3), ("W_P1", CUR_ID + 1)):
        kf_id[b.name[n]] = v
    if wrap:                                                          # the window test at the top of the unsigned range: W_M2's id + 2 wraps to 0
        for n, v in (("CUR", 2 ** 32 - 1), ("W_AT", 2 ** 32 - 1), ("W_M2", 2 ** 32 - 2), ("W_M3", 2 ** 32 - 3), ("W_P1", 0)):
            kf_id[b.name[n]] = v
    kf_erased = np.zeros(F, np.uint8); kf_erased[e] = 1
    cannot = np.zeros(F, np.uint8); cannot[b.name["HELD"]] = 1
    lm_erased = (rng.integers(0, 25, L) == 0).astype(np.uint8)
    lm_erased[n_base:] = 0
    if setup:                                                         # the depth gates: below 0, above the key frame's threshold, NaN
        for f in range(b.base):
            for idx, v in zip(rng.permutation(int(b.counts[f]))[:6], (-1.0, -0.5, 50.0, 41.0, np.nan, np.nan)):
                b.depths[f, idx] = v
        b.depth_thr[:b.base] = rng.uniform(35.0, 45.0, b.base)
    offsets = np.zeros(L + 1, np.int32)
    offsets[1:] = np.cumsum([len(o) for o in b.obs])
    flat = [t for o in b.obs for t in o]
    obs_kf = np.array([t[0] for t in flat], np.int32)
    obs_idx = np.array([t[1] for t in flat], np.int32)
    kf_lm = b.kf_lm
    if outside:                                                       # rows outside their tables: empty slots, absent observations
        kf_lm = kf_lm.copy()
        empty = np.argwhere(kf_lm[:b.base, :60] < 0)[:6]
        for (f, idx), v in zip(empty, (L, L + 9, -2, -1000, 2 ** 31 - 1, -2 ** 31)):
            kf_lm[f, idx] = v
    sc = dict(setup=setup, is_monocular=int(setup == 0), origin_id=ORIGIN_ID, kf_lm=kf_lm, kf_counts=b.counts, undist=b.undist,
              x_right=b.x_right if setup else None, depths=b.depths if setup else None, depth_thr=b.depth_thr if setup else None, kf_id=kf_id,
              kf_erased=kf_erased, kf_cannot_erase=cannot, obs_offsets=offsets, obs_kf=obs_kf, obs_idx=obs_idx, lm_erased=lm_erased, lm_num_obs=None,
              names=b.name, base=b.base)
    if outside:                                                       # three observations more per list head, none of them in the tables
        sc["obs_kf"], sc["obs_idx"], sc["obs_offsets"] = _absent_observations(sc, F, cap)
    cur, off, cv = [], [0], []
    for c, lst in problems(b, rng):
        cur.append(b.name.get(c, c))
        cv += [b.name.get(v, v) for v in lst]
        off.append(len(cv))
    sc.update(cur_kf=np.array(cur, np.int32), covis_offsets=np.array(off, np.int32), covis=np.array(cv, np.int32))
    if lm_num_obs:                                                    # num_observations_ as the reference keeps it: equal to the derived one
        n = np.zeros(L, np.uint32)
        for lm in range(L):
            for t in range(int(sc["obs_offsets"][lm]), int(sc["obs_offsets"][lm + 1])):
                kf, idx = int(sc["obs_kf"][t]), int(sc["obs_idx"][t])
                if 0 <= kf < F and 0 <= idx < cap:
                    n[lm] += 2 if setup and b.x_right[kf, idx] >= 0 else 1
        sc["lm_num_obs"] = n
    return sc


def _absent_observations(sc, F, cap):
    """the lists of the first three landmarks that have one, each with an entry whose key frame or index is outside the tables"""
    kf, idx, off = list(sc["obs_kf"]), list(sc["obs_idx"]), list(sc["obs_offsets"])
    done = 0
    for lm in range(len(off) - 1):
        if off[lm + 1] > off[lm] and done < 3:
            at = off[lm] + 1
            kf.insert(at, (F, -1, 3)[done]); idx.insert(at, (0, 0, cap)[done])
            for m in range(lm + 1, len(off)):
                off[m] += 1
            done += 1
    return np.array(kf, np.int32), np.array(idx, np.int32), np.array(off, np.int32)


def _main_list(b, rng, tail):
    head = ["ORIGIN", "W_AT", "W_M2", "W_M3", "W_P1", "EMPTY", "K910", "K89", "HELD", "ERASED", "Z", "FLIP_RK", "FLIP_KR"]
    return head + [int(v) for v in rng.permutation(b.base)[:tail]]


def _one(b, rng):
    return [("CUR", _main_list(b, rng, 60))]                          # 73 entries: longer than a wave


def _several(b, rng):
    """ragged lists, an empty one, one entry, a current key frame and an entry outside the table"""
    return [("CUR", _main_list(b, rng, 20)), ("CUR2", []), ("CUR", ["Z"]), ("CUR2", ["FLIP_KR", "Z", "FLIP_RK", b.F + 3, -1] + list(range(5))),
            (b.F, ["Z", "K910"]), ("CUR2", ["K910", "Z", "HELD", "FLIP_RK", "FLIP_KR"] + [int(v) for v in rng.permutation(b.base)[:70]])]


def _several_inside(b, rng):
    """_several with every row inside the table: what a build of the reference, which follows pointers, can be handed whole"""
    return [(c, [v for v in lst if b.name.get(v, v) in range(b.F)]) for c, lst in _several(b, rng) if b.name.get(c, c) in range(b.F)]


def _short(b, rng):
    return [("CUR", _main_list(b, rng, 12))]


# stereo97c is stereo97 without a row outside a table; wrap65 has the ids of the window's key frames at the top of the unsigned range: W_M2 is
# 2^32 - 2 against a current key frame of 2^32 - 1, so `id + 2` wraps to 0 and the entry is counted and removed (signed arithmetic would skip it)
_SPECS = dict(mono97=dict(F=97, setup=0, seed=11, problems=_one),
              mono65=dict(F=65, setup=0, seed=12, problems=_several, lm_num_obs=True),
              stereo97=dict(F=97, setup=1, seed=13, problems=_several, outside=True),
              rgbd65=dict(F=65, setup=2, seed=14, problems=_one, lm_num_obs=True),
              stereo97c=dict(F=97, setup=1, seed=13, problems=_several_inside),
              wrap65=dict(F=65, setup=0, seed=15, problems=_short, wrap=True))
SCENES = tuple(_SPECS)
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = keyframe_scene(**_SPECS[name])
    return _cache[name]


KF_TABLES = ("kf_lm", "kf_counts", "undist", "x_right", "depths", "depth_thr", "kf_id", "kf_erased", "kf_cannot_erase", "obs_offsets", "obs_kf", "obs_idx",
             "lm_erased", "lm_num_obs", "cur_kf", "covis_offsets", "covis")


def call_args(sc, **over):
    """the keyword arguments of matcher.cull_keyframes / model_cull_keyframes for a scene"""
    a = {k: sc[k] for k in KF_TABLES}
    a.update(origin_id=sc["origin_id"], is_monocular=bool(sc["is_monocular"]))
    a.update(over)
    return a


def landmark_scene(seed, lines):
    """R = 5 fresh lists over one table: designed rows for every branch of :73-110 and its bounds, then random ones; the lists are 0, 1, 70, 300
    and 257 entries long, so they end mid-wave, cross the workgroup of 256 and end one past it"""
    rng = np.random.default_rng(seed)
    cur = 50
    rows = []   # (erased, observed, observable, first, num_obs, plane)
    rows += [(1, 9, 10, 0, 9, 0), (0, 1, 10, 0, 9, 0), (0, 1, 10, 0, 9, 1), (0, 0, 0, 0, 9, 0), (0, 5, 0, 0, 9, 0), (0, 3, 10, 0, 9, 0), (0, 29, 100, 0, 9, 0)]
    for first in (cur - 2, cur - 3, cur - 1, cur - 4):
        for n in (2, 3, 4):
            for plane in (0, 1):
                rows.append((0, 9, 10, first, n, plane))
    rows.append((0, 9, 10, 2 ** 32 - 2, 1, 0))                         # 2 + first wraps to 0
    for _ in range(700):
        rows.append((int(rng.integers(0, 12) == 0), int(rng.integers(0, 12)), int(rng.integers(0, 12)), int(rng.integers(cur - 6, cur + 2)),
                     int(rng.integers(0, 7)), int(rng.integers(0, 5) == 0)))
    t = np.array(rows, np.int64)
    L = len(rows)
    lists = [[], [3], list(range(40)) + [int(v) for v in rng.integers(0, L, 30)], [int(v) for v in rng.permutation(L)[:300]],
             [L, -1] + [int(v) for v in rng.integers(0, L, 255)]]
    off = np.cumsum([0] + [len(v) for v in lists]).astype(np.int32)
    return dict(fresh_offsets=off, fresh=np.array([v for l in lists for v in l], np.int32), lm_erased=t[:, 0].astype(np.uint8),
                num_observed=t[:, 1].astype(np.uint32), num_observable=t[:, 2].astype(np.uint32), first_kf_id=t[:, 3].astype(np.uint32),
                num_obs=t[:, 4].astype(np.uint32), owning_plane=None if lines else t[:, 5].astype(np.uint8),
                cur_kf_id=np.array([cur, cur, cur, cur, cur + 1], np.uint32), num_obs_thr=np.array([3] * 5 if lines else [2, 3, 2, 3, 3], np.uint32))


LM_SCENES = dict(points=dict(seed=21, lines=False), lines=dict(seed=22, lines=True))
LM_TABLES = ("fresh_offsets", "fresh", "num_observed", "num_observable", "first_kf_id", "num_obs", "cur_kf_id", "num_obs_thr", "lm_erased", "owning_plane")


def lm_scene(name):
    if ("lm", name) not in _cache:
        _cache[("lm", name)] = landmark_scene(**LM_SCENES[name])
    return _cache[("lm", name)]


def lm_call_args(sc, **over):
    a = {k: sc[k] for k in LM_TABLES}
    a.update(over)
    return a
