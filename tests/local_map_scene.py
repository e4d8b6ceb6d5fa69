"""Seeded map snapshots with B ragged frames for the local-map tests (plp_local_map_*): small on purpose, with every
table carrying the irregular entries D18 names -- erased key frames and landmarks, rows outside their table, duplicates inside and across key
frames, counts below the row width with valid-looking rows behind them, observation runs of 0, 1 and more than 64 entries, a frame without a
landmark, a frame whose voted key frames are all erased.  The census of tests/test_local_map_cpu.py says which branches SCENES reaches."""
import numpy as np

i32, u8 = np.int32, np.uint8


def make_scene(seed, F, cap, fcap, L=400, LL=120, lcap=9, flcap=7, B=5, max_kf=60, stride_pad=0, lines=True, spread=4):
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
        kf_lm_lines = ((np.arange(F)[:, None] * LL // max(F, 1) + rng.integers(-5, 6, (F, lcap))) % LL).astype(i32)
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


def scene(name):
    """the scene of that name, made once and shared: treat it as read-only"""
    if name not in _cache:
        _cache[name] = make_scene(**SCENES[name])
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
