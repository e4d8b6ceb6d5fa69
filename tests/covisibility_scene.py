"""Small seeded map snapshots for the covisibility graph: numpy tables in the layout of plp_covisibility_update_args, a
previous snapshot from which the graph's initial state is grown, and the owner lists and erase masks the tests run.

A scene is two snapshots of one map.  `prev` is the map before the newest key frames existed and before a fusion erased landmarks; the initial
state is update_connections() of every key frame over `prev`, by the restatement.  The calls under test run over the current snapshot, so the
graph they meet holds stale weights, connections of equal weight, parents that are set and parents that are not.

  F      5 (below a wave; weights designed: 14, 15, 16, 17, ties, a key frame with nothing above the threshold), 70 (above a wave), 300 (above a
         stride of 256 lanes), 1100 (above a stride of 1024)
  cap    48 - 96 slots; observation lists of 0 - 40 entries
"""
import numpy as np

import covisibility_ref as R

SIZES = dict(f5=(5, 96, 11), f70=(70, 64, 12), f300=(300, 48, 13), f1100=(1100, 56, 14))
SCENES = tuple(SIZES)
TABLES = ("kf_lm", "kf_counts", "obs_offsets", "obs_kf", "lm_erased", "kf_id")
_cache = {}


def _designed(F, cap):
    """F = 5: landmarks seen by exactly two key frames, as many as the weight wanted"""
    want = {(0, 1): 16, (0, 2): 15, (0, 3): 14, (0, 4): 17, (1, 2): 16, (1, 3): 3, (3, 4): 15, (2, 4): 16}
    return [[a, b] for (a, b), n in want.items() for _ in range(n)] + [[2], []]


def _random(F, cap, rng):
    """observation lists of 0 - 40 key frames out of a window of the map, until the rows are four fifths full"""
    free = np.full(F, int(cap * 0.8))
    lists = []
    while free.sum() > F * cap * 0.05 and len(lists) < F * cap:
        n = int(min(rng.geometric(0.18) - 1, 40)) if rng.random() > 0.02 else 40
        c, w = int(rng.integers(F)), int(rng.choice([2, 4, 8, 24]))
        cand = np.arange(max(c - w, 0), min(c + w + 1, F))
        cand = cand[free[cand] > 0]
        obs = rng.choice(cand, min(n, len(cand)), replace=False) if len(cand) else np.zeros(0, np.int64)
        free[obs] -= 1
        lists.append([int(v) for v in obs])
    return lists


def _build(name):
    """name: one of SCENES, or (F, cap, seed) with F > 5 for a map of another size"""
    F, cap, seed = SIZES[name] if isinstance(name, str) else name
    rng = np.random.default_rng(seed)
    lists = _designed(F, cap) if F == 5 else _random(F, cap, rng)
    L = len(lists)
    kf_lm = np.full((F, cap), -1, np.int32)
    order = [list(rng.permutation(cap)) for _ in range(F)]           # the slots of a key frame are taken in a random order
    for lm, obs in enumerate(lists):
        for kf in obs:
            kf_lm[kf, order[kf].pop()] = lm
    obs_offsets = np.concatenate([[0], np.cumsum([len(o) for o in lists])]).astype(np.int32)
    obs_kf = np.array([kf for o in lists for kf in o], np.int32)
    s = 0 if F == 5 else F // 5                                      # the pair (s, s + 1) shares nothing after the fusion
    z = None if F == 5 else F // 2                                   # a key frame without a slot of its own that others observe with
    new = [F - 1] if F == 5 else [F - 1, F - 3]                      # the key frames the previous snapshot does not have
    kf_id = (np.arange(F) + 100).astype(np.uint32)
    kf_id[1] = 0
    kf_counts = np.full(F, cap, np.int32)
    kf_counts[F - 2] = cap + 9                                       # cut to the cap
    # ---- the previous snapshot
    prev_counts = kf_counts.copy()
    prev_counts[new] = 0
    prev_obs = obs_kf.copy()
    prev_obs[np.isin(obs_kf, new)] = -1
    prev = dict(kf_lm=kf_lm.copy(), kf_counts=prev_counts, obs_offsets=obs_offsets, obs_kf=prev_obs, lm_erased=np.zeros(L, np.uint8), kf_id=kf_id)
    # ---- the current one: the fusion, and what a table can hold that the text skips
    lm_erased = (rng.random(L) < 0.03).astype(np.uint8)
    for lm, obs in enumerate(lists):
        if s in obs and s + 1 in obs:
            lm_erased[lm] = 1
    if z is not None:
        kf_counts[z] = 0
        kf_counts[z + 3] = -4                                        # cut to 0 as well
    for k in range(0, F, 3 if F > 5 else 1):
        slots = order[k]
        if len(slots) >= 3:
            kf_lm[k, slots.pop()] = L + 3                            # rows outside the table
            kf_lm[k, slots.pop()] = -5
            held = kf_lm[k][(kf_lm[k] >= 0) & (kf_lm[k] < L)]
            if len(held):
                kf_lm[k, slots.pop()] = held[int(rng.integers(len(held)))]   # a landmark in two slots
    cur_obs = obs_kf.copy()
    hit = rng.random(len(cur_obs)) < 0.01
    cur_obs[hit] = np.where(rng.random(int(hit.sum())) < 0.5, F + 2, -3)
    sc = dict(name=name, kf_lm=kf_lm, kf_counts=kf_counts, obs_offsets=obs_offsets, obs_kf=cur_obs, lm_erased=lm_erased, kf_id=kf_id, prev=prev,
              s=s, z=z, new=new)
    # ---- the initial state
    g = R.graph(F)
    R.run_update(g, prev, range(F))
    sc["graph"] = g
    # ---- the problems
    perm = [int(v) for v in rng.permutation(F)]
    sc["owners"] = dict(one=[F - 1], three=[F - 1, F - 3, F - 2] if F > 5 else [4, 2, 0], all=perm, stale=[s])
    a = F // 4 if F > 5 else 2
    sc["erase"] = dict(one=[s], pair=[a, a + 1] if F > 5 else [2, 4], many=[int(v) for v in rng.permutation(F)[:max(F // 8, 2)]])
    return sc


def scene(name):
    if name not in _cache:
        _cache[name] = _build(name)
    return _cache[name]


def call_args(sc, **over):
    """the snapshot as the keyword arguments of model_covisibility_update / matcher.covisibility_update"""
    a = {k: sc[k] for k in TABLES}
    a.update(over)
    return a


def caps(g):
    """row lengths that hold every list of the graph, and then some"""
    return max(len(c) for c in g.connected) + 3, max(max(len(o) for o in g.ordered), 10) + 2
