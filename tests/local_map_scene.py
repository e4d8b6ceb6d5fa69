"""Seeded map snapshots with B ragged frames for the local-map tests (plp_local_map_*): small on purpose, with every
table carrying the irregular entries D18 names -- erased key frames and landmarks, rows outside their table, duplicates inside and across key
frames, counts below the row width with valid-looking rows behind them, observation runs of 0, 1 and more than 64 entries, a frame without a
landmark, a frame whose voted key frames are all erased.  The census of tests/test_local_map_cpu.py says which branches SCENES reaches.
WIDE_SCENES are the same kind of map at the widths where a workgroup of the kernels takes a second pass; tests/test_local_map_wide_cpu.py has
their census."""
import numpy as np

i32, u8 = np.int32, np.uint8


def make_scene(seed, F, cap, fcap, L=400, LL=120, lcap=9, flcap=7, B=5, max_kf=60, stride_pad=0, lines=True, spread=4, line_spread=5):
    rng = np.random.default_rng(seed)
    kf_erased = (rng.random(F) < 0.1).astype(u8)
    gone = int(rng.integers(F)) if F >= 3 else -1            # a key frame that is surely erased, with landmarks of its own
    if gone >= 0:
        kf_erased[gone] = 1
    lm_erased = (rng.random(L) < 0.08).astype(u8)
    own = list(range(L - 6, L)) if gone >= 0 else []          # the landmarks only `gone` observes
    lm_erased[L - 6:] = 0

    # observation lists: runs of 0, 1, a few and 70 entries around a centre key frame
    centre = rng.integers(0, F, L)
    obs_offsets, obs_kf, obs_idx = [0], [], []
    kf_lm = np.full((F, cap), -1, i32)
    used = np.zeros(F, i32)
    for l in range(L):
        u = rng.random()
        n = 0 if u < 0.1 else 1 if u < 0.25 else int(rng.integers(2, 9))
        if l % 97 == 5:
            n = 70
        lo, hi = max(0, centre[l] - spread), min(F, centre[l] + spread + 1)
        if n == 70:
            lo, hi = 0, F
        kfs = rng.choice(np.arange(lo, hi), size=n, replace=n > hi - lo)
        if l in own:
            kfs = np.full(1 + l % 3, gone)
        for kf in kfs.tolist():
            idx = -1
            if used[kf] < cap:
                idx = int(used[kf])
                kf_lm[kf, idx] = l
                used[kf] += 1
            if rng.random() < 0.02:
                kf = F + 3 if rng.random() < 0.5 else -4       # outside the table
            obs_kf.append(kf)
            obs_idx.append(idx)
        obs_offsets.append(len(obs_kf))
    # counts: a little past the used slots, junk in between, valid-looking rows behind the count
    kf_counts = np.minimum(cap, used + rng.integers(0, 3, F)).astype(i32)
    for kf in range(F):
        for idx in range(int(used[kf]), int(kf_counts[kf])):
            kf_lm[kf, idx] = [-1, kf_lm[kf, 0], int(rng.integers(L)), L + 7, -9][int(rng.integers(5))]
        kf_lm[kf, int(kf_counts[kf]):] = rng.integers(0, L, cap - int(kf_counts[kf]))
    if F >= 65:
        kf_counts[7], kf_counts[9] = cap + 5, -2                # cut to [0, cap]
        kf_lm[9, :] = rng.integers(0, L, cap)

    # covisibilities, spanning tree
    kf_covis = np.full((F, 10), -1, i32)
    kf_parent = np.full(F, -1, i32)
    for kf in range(F):
        n = int(rng.integers(0, 11))
        row = (kf + rng.integers(-12, 13, n)) % F
        far = rng.random(n) < 0.2
        row[far] = rng.integers(0, F, int(far.sum()))
        bad = rng.random(n)
        row[bad < 0.03] = F + 1
        row[(bad >= 0.03) & (bad < 0.06)] = -3
        row[(bad >= 0.06) & (bad < 0.10)] = -1
        kf_covis[kf, :n] = row
        if kf > 0 and rng.random() < 0.9:
            kf_parent[kf] = int(rng.integers(max(0, kf - 6), kf))
        if rng.random() < 0.04:
            kf_parent[kf] = F + 2
    kids = [[] for _ in range(F)]
    for kf in range(F):
        if 0 <= kf_parent[kf] < F:
            kids[kf_parent[kf]].append(kf)
    kf_children_offsets, kf_children = [0], []
    for kf in range(F):
        c = kids[kf]
        rng.shuffle(c)
        if rng.random() < 0.05:
            c = [F + 9] + c + [-5]
        kf_children += c
        kf_children_offsets.append(len(kf_children))

    # lines: no votes, so any table will do
    kf_lm_lines = kf_kl_counts = lm_erased_lines = frm_lm_lines = frm_kl_counts = None
    if lines:
        kf_lm_lines = ((np.arange(F)[:, None] * LL // max(F, 1) + rng.integers(-line_spread, line_spread + 1, (F, lcap))) % LL).astype(i32)
        junk = rng.random((F, lcap))
        kf_lm_lines[junk < 0.4] = -1
        kf_lm_lines[(junk >= 0.4) & (junk < 0.43)] = LL + 4
        kf_kl_counts = rng.integers(0, lcap + 1, F).astype(i32)
        lm_erased_lines = (rng.random(LL) < 0.1).astype(u8)
        frm_lm_lines = rng.integers(-1, LL, (B, flcap + stride_pad)).astype(i32)
        frm_lm_lines[rng.random(frm_lm_lines.shape) < 0.3] = -1
        frm_lm_lines[0, 0] = LL + 1
        frm_kl_counts = rng.integers(0, flcap + 1, B).astype(i32)

    # frames: 0 votes everywhere, 1 in a window of key frames, 2 narrowly, 3 holds nothing, 4 only what `gone` observes, 5 that and two more
    frm_lm = rng.integers(0, L, (B, fcap + stride_pad)).astype(i32)            # valid-looking rows behind the counts and the row
    frm_counts = np.zeros(B, i32)
    for b in range(B):
        kind = b % 6
        n = fcap if kind == 0 else int(rng.integers((fcap + 1) // 2, fcap + 1))
        width = [F, 26, 3, 0, 0, 0][kind]
        c0 = int(rng.integers(F))
        pool = np.flatnonzero(np.abs(centre - c0) <= width)
        row = rng.choice(pool, n) if len(pool) and kind <= 2 else np.full(n, -1)
        if kind == 3:
            row = np.full(n, -1)
        if kind >= 4 and own:
            row = rng.choice(own, n)
            if kind == 5 and n >= 3:
                row[:2] = rng.choice(np.flatnonzero(lm_erased[:L - 6] == 0), 2)
        row = row.astype(i32)
        junk = rng.random(n)
        if kind <= 2:
            row[junk < 0.08] = -1
            row[(junk >= 0.08) & (junk < 0.10)] = L + 11
            row[(junk >= 0.10) & (junk < 0.12)] = -6
        frm_lm[b, :n] = row
        frm_counts[b] = n
    return dict(seed=seed, cap=cap, lcap=lcap if lines else 0, fcap=fcap, flcap=flcap if lines else 0, LL=LL if lines else 0, max_kf=max_kf,
                kf_erased=kf_erased, kf_covis=kf_covis, kf_parent=kf_parent, kf_children_offsets=np.array(kf_children_offsets, i32),
                kf_children=np.array(kf_children, i32), kf_lm=kf_lm, kf_counts=kf_counts, kf_lm_lines=kf_lm_lines, kf_kl_counts=kf_kl_counts,
                obs_offsets=np.array(obs_offsets, i32), obs_kf=np.array(obs_kf, i32), obs_idx=np.array(obs_idx, i32), lm_erased=lm_erased,
                lm_erased_lines=lm_erased_lines, frm_lm=frm_lm, frm_counts=frm_counts, frm_lm_lines=frm_lm_lines, frm_kl_counts=frm_kl_counts)


# name -> make_scene arguments; F in {1, 63, 64, 65, 130}, cap and fcap in {1, 63, 64, 65, 70}
SCENES = {
    "f130": dict(seed=1, F=130, cap=70, fcap=70, L=600, B=6),
    "f130_mid": dict(seed=2, F=130, cap=63, fcap=65, L=600, B=6, spread=2),
    "f65": dict(seed=3, F=65, cap=65, fcap=64, L=300, B=6, max_kf=20, stride_pad=3),
    "f64": dict(seed=4, F=64, cap=64, fcap=63, L=300, B=5, max_kf=12, lcap=1, flcap=1),
    "f63": dict(seed=5, F=63, cap=1, fcap=70, L=200, B=6, max_kf=9),
    "f63_points": dict(seed=6, F=63, cap=63, fcap=1, L=200, B=4, lines=False),
    "f1": dict(seed=7, F=1, cap=64, fcap=65, L=40, LL=10, B=3),
}
_cache = {}


# ---- the wide scenes: every loop of csrc/local_map.hpp that strides by the team takes a second pass on the device (512 lanes over key frames,
# frame slots and candidates, 256 over the slots a block marks, 64 over a children run).  make_scene gives the bulk; what an edge needs for
# certain is placed by hand afterwards, on the tables alone, so that no seed has to be lucky.
def frame_weights(sc, b):
    """the votes of frame b per key frame, counted in numpy: the edits below place ties and lone votes with it"""
    F, L = len(sc["kf_parent"]), len(sc["obs_offsets"]) - 1
    n = min(max(int(sc["frm_counts"][b]), 0), sc["fcap"])
    row = sc["frm_lm"][b, :n]
    row = row[(row >= 0) & (row < L)]
    row = row[sc["lm_erased"][row] == 0]
    w = np.zeros(F, np.int64)
    for lm in row.tolist():
        kfs = sc["obs_kf"][sc["obs_offsets"][lm]:sc["obs_offsets"][lm + 1]]
        np.add.at(w, kfs[(kfs >= 0) & (kfs < F)], 1)
    return w


def add_landmarks(sc, runs):
    """append one landmark per observation run (a list of key-frame rows), held by no key frame; returns their rows"""
    L = len(sc["obs_offsets"]) - 1
    off, kfs = sc["obs_offsets"].tolist(), sc["obs_kf"].tolist()
    for run in runs:
        kfs += list(run)
        off.append(len(kfs))
    more = len(kfs) - len(sc["obs_kf"])
    sc["obs_offsets"], sc["obs_kf"] = np.array(off, i32), np.array(kfs, i32)
    sc["obs_idx"] = np.concatenate([sc["obs_idx"], np.full(more, -1, i32)])
    sc["lm_erased"] = np.concatenate([sc["lm_erased"], np.zeros(len(runs), u8)])
    return list(range(L, L + len(runs)))


def force_heaviest(sc, b, kfs):
    """give every key frame of `kfs` the same weight in frame b, above every other: the last slots below the frame's count are emptied, as many as
    that can take, then filled with copies of one new landmark per key frame that only it observes"""
    n = int(sc["frm_counts"][b])
    top = int(frame_weights(sc, b).max()) + 2
    room = len(kfs) * top
    assert n >= room and all(sc["kf_erased"][kf] == 0 for kf in kfs)
    sc["frm_lm"][b, n - room:n] = -1
    w = frame_weights(sc, b)
    lms = add_landmarks(sc, [[kf] for kf in kfs])
    s = n - room
    for kf, lm in zip(kfs, lms):
        k = top - int(w[kf])
        assert s + k <= n
        sc["frm_lm"][b, s:s + k] = lm
        s += k


def lone_vote(sc, b, slot, kf):
    """make slot `slot` of frame b the only vote for key frame kf: the frame's other slots that vote for it are emptied"""
    n, L = int(sc["frm_counts"][b]), len(sc["obs_offsets"]) - 1
    assert slot < n and sc["kf_erased"][kf] == 0
    for s in range(n):
        lm = int(sc["frm_lm"][b, s])
        if 0 <= lm < L and (sc["obs_kf"][sc["obs_offsets"][lm]:sc["obs_offsets"][lm + 1]] == kf).any():
            sc["frm_lm"][b, s] = -1
    sc["frm_lm"][b, slot] = add_landmarks(sc, [[kf]])[0]


def live_rows(sc, lo, hi):
    return [kf for kf in range(lo, hi) if sc["kf_erased"][kf] == 0]


def _wide_f():
    """F = 1100: three passes of 512 over the key frames and 18 tiles of the walk.  Frame 0 votes everywhere and has its largest weight twice, at
    a row below 512 and at one above; frame 1 has it twice inside the second pass, in different waves; frame 2 once, in the third pass"""
    sc = make_scene(seed=21, F=1100, cap=32, fcap=600, L=6000, B=6, max_kf=5000, spread=40)
    force_heaviest(sc, 0, [live_rows(sc, 300, 512)[0], live_rows(sc, 700, 1024)[0]])
    force_heaviest(sc, 1, [live_rows(sc, 530, 576)[0], live_rows(sc, 900, 960)[0]])
    force_heaviest(sc, 2, [live_rows(sc, 1050, 1100)[0]])
    return sc


def _wide_f_cut():
    """the same map with max_kf between 512 and frame 0's first local key frames: the walk stops before its first iteration only if `n` was
    carried over the passes"""
    return dict(scene("wide_f"), max_kf=600)


def _deep_kf():
    """cap = 600: a key frame's slots take three passes of the mark kernel's 256 lanes and two of the compaction's 512"""
    return make_scene(seed=22, F=70, cap=600, fcap=70, L=9000, B=6)


def _deep_lines():
    """the same widths on the line side, with more line rows than point rows: the mark table is as wide as LL"""
    sc = make_scene(seed=23, F=70, cap=20, fcap=30, L=400, LL=3008, lcap=600, flcap=600, B=6, stride_pad=2, line_spread=400)
    sc["frm_kl_counts"][:4] = [600, 513, 512, 257]
    sc["kf_kl_counts"][live_rows(sc, 0, 70)[:8]] = [600, 513, 512, 511, 257, 256, 255, 600]
    return sc


def _deep_frame():
    """fcap = 1100 with counts of 1100, 512, 513 and 511 and padded rows; in every frame the last slot below the count is some key frame's only
    vote, in frame 0 slot 512 is another's"""
    sc = make_scene(seed=24, F=70, cap=200, fcap=1100, L=3000, B=4, stride_pad=5)
    sc["frm_lm"][3] = sc["frm_lm"][0]
    sc["frm_counts"][:] = [1100, 512, 513, 511]
    live = live_rows(sc, 0, 70)
    lone_vote(sc, 0, 1099, live[0])
    lone_vote(sc, 0, 512, live[1])
    lone_vote(sc, 1, 511, live[2])
    lone_vote(sc, 2, 512, live[3])
    lone_vote(sc, 3, 510, live[4])
    return sc


def _hub():
    """four first local key frames of one frame with long children runs: 200 children of which the first 64 are rejected (erased, local already,
    outside the table) and the one at position 64 is taken; 140 with the first acceptable one at position 130; 70 that are all rejected, so that
    the parent is tried and taken; 200 that are all rejected.  The hubs' own covisibilities are empty, so nothing but their children and parents is added for them"""
    sc = make_scene(seed=25, F=200, cap=20, fcap=40, L=600, B=4, max_kf=1000)
    F = 200
    for b in range(1, 4):                                     # the frame whose votes leave key frames to accept
        w = frame_weights(sc, b)
        first = [kf for kf in range(F) if w[kf] > 0 and sc["kf_erased"][kf] == 0]
        free = [kf for kf in range(F) if w[kf] == 0 and sc["kf_erased"][kf] == 0]
        if len(first) >= 30 and len(free) >= 3:
            break
    else:
        raise AssertionError("no frame for the hubs")
    hubs, take = first[:4], free[:3]
    gone = np.flatnonzero(sc["kf_erased"]).tolist()
    bad = []                                                    # a mix of rejected children: local already, erased, outside the table
    for i in range(200):
        bad.append([first[4 + i % (len(first) - 4)], gone[i % len(gone)], F + 9, -5, -1][i % 5] if i % 2 else first[4 + i % (len(first) - 4)])
    runs = {hubs[0]: bad[:64] + [take[0]] + bad[64:199], hubs[1]: bad[:130] + [take[1]] + bad[130:139] + [take[0]], hubs[2]: bad[:69] + [take[0]], hubs[3]: bad}
    off, kids = sc["kf_children_offsets"].tolist(), sc["kf_children"].tolist()
    new_off, new_kids = [0], []
    for kf in range(F):
        new_kids += runs.get(kf, kids[off[kf]:off[kf + 1]])
        new_off.append(len(new_kids))
    sc["kf_children_offsets"], sc["kf_children"] = np.array(new_off, i32), np.array(new_kids, i32)
    sc["kf_covis"][hubs] = -1
    sc["kf_parent"][hubs] = [-1, -1, take[2], -1]
    return sc


def _hot():
    """all 8192 slots of frame 0 hold one landmark that one key frame observes once: 8192 adds on one counter, a weight of exactly 8192"""
    sc = make_scene(seed=26, F=5, cap=8, fcap=8192, L=40, LL=10, lcap=3, flcap=3, B=2)
    sc["kf_erased"][1] = 0
    sc["frm_lm"][0, :8192] = add_landmarks(sc, [[1]])[0]
    return sc


def _f_max():
    """F = 8192, the whole weight table and bitmap: frame 0 votes for rows 0, 100, 7700 and 8191 among others, 8191 is its heaviest, and the walk runs over all 128 tiles"""
    sc = make_scene(seed=27, F=8192, cap=4, fcap=64, L=300, B=2, max_kf=9000)
    rows = [0, 100, 7700, 8191]
    sc["kf_erased"][rows] = 0
    sc["frm_lm"][0, :4] = add_landmarks(sc, [[kf] for kf in rows])
    force_heaviest(sc, 0, [8191])
    return sc


def _cap_max(L):
    """cap = 8192 with every slot of the three key frames used, none erased: the positions k * cap + idx go up to 3 * 8192 - 1, and that last slot
    holds a landmark seen nowhere else.  The last row of the landmark table is in the list and the frame holds it: the last bit of the bitmap"""
    def make():
        sc = make_scene(seed=28, F=3, cap=8192, fcap=64, L=L, B=2)
        sc["kf_erased"][:] = 0
        assert (sc["kf_counts"] == 8192).all()
        fresh = [lm for lm in range(L - 6) if sc["lm_erased"][lm] == 0 and not (sc["kf_lm"] == lm).any()][0]
        sc["kf_lm"][2, 8191] = fresh
        sc["kf_lm"][0, 100] = L - 1
        sc["frm_lm"][0, 3] = L - 1
        return sc
    return make


# name -> builder
WIDE_SCENES = {
    "wide_f": _wide_f, "wide_f_cut": _wide_f_cut, "deep_kf": _deep_kf, "deep_lines": _deep_lines, "deep_frame": _deep_frame, "hub": _hub,
    "hot": _hot, "f_max": _f_max, "cap_max": _cap_max(8192 + 32), "cap_max_less": _cap_max(8192 + 31), "cap_max_more": _cap_max(8192 + 33),
}


def scene(name):
    """the scene of that name, made once and shared: treat it as read-only"""
    if name not in _cache:
        _cache[name] = make_scene(**SCENES[name]) if name in SCENES else WIDE_SCENES[name]()
    return _cache[name]


def call_args(sc, **over):
    """the keyword arguments of plp.model_local_map / matcher.local_map for a scene"""
    a = dict(kf_covis=sc["kf_covis"], kf_parent=sc["kf_parent"], kf_children_offsets=sc["kf_children_offsets"], kf_children=sc["kf_children"],
             kf_lm=sc["kf_lm"], obs_offsets=sc["obs_offsets"], obs_kf=sc["obs_kf"], frm_lm=sc["frm_lm"], kf_erased=sc["kf_erased"],
             kf_counts=sc["kf_counts"], kf_lm_lines=sc["kf_lm_lines"], kf_kl_counts=sc["kf_kl_counts"], lm_erased=sc["lm_erased"],
             lm_erased_lines=sc["lm_erased_lines"], LL=sc["LL"], frm_counts=sc["frm_counts"], frm_lm_lines=sc["frm_lm_lines"],
             frm_kl_counts=sc["frm_kl_counts"], max_num_local_keyfrms=sc["max_kf"], fcap=sc["fcap"], flcap=sc["flcap"])
    a.update(over)
    return a
