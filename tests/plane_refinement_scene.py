"""Seeded scenes for the plane refinement: small maps built for the branches of merge_planes, refine_planes and
refine_points.  A scene is a list of plane specs over a catalogue of generating planes; `build` turns one into the tables of one problem, `pack`
several into the arrays of a call (padded to common caps: padding plane rows have state 0, padding landmarks are erased, unused slots hold -9)."""
import numpy as np

import plane_ransac_ref as PR
import plane_refinement_ref as RR

DIST, ERR = 0.02, 0.002                 # _planar_distance_thresh, _final_error_thresh of the scenes
PPR, ITERS, DOT, FACTOR, SEED = 18, 8, 0.8, 6, 5
NOISE, FAR = DIST / 4, 4 * DIST         # the margins of D19: noise <= 1/4 threshold, outliers >= 4 thresholds
IN_DB, VALID, NEED = RR.IN_DB, RR.VALID, RR.NEED
LIVE = IN_DB | VALID                    # a plane that was fitted and refined
NEW = IN_DB | VALID | NEED              # ... that create_new_plane just added
DEAD = IN_DB                            # ... that was invalidated and not yet erased
PAD = -9

# generating planes (unit normal, d): 0 and 1 differ in offset and angle, 2 is parallel to 0 and far, 3 has 0's offset and another angle
GEN = [((0.0, 0.0, 1.0), -1.0), ((1.0, 0.0, 0.0), -3.0), ((0.0, 0.0, 1.0), -2.0), ((1.0, 0.0, 0.0), -1.0), ((0.0, 1.0, 0.0), 2.0), ((0.0, 0.6, 0.8), -5.0)]


def P(gen, n, state=LIVE, **kw):
    """a plane spec: n members sampled from generating plane gen.  share: the first `share` members are the LAST members of the previous spec;
    outliers / erased / unowned: how many of the own members (from the end) are far off (FAR .. far * FAR) / will_be_erased / have no owner; nan: one member's
    position is NaN (slot `nan`, or chosen by nan_last: the last hypothesis of update call c draws it, an earlier one does not);
    foreign: members owned by the previous row; eq: the row's equation, default the generating plane's; best_error: default 1.0"""
    return dict(gen=gen, n=n, state=state, **kw)


def build(spec, rng, g=0, seed=SEED):
    """the tables of one problem (no problem axis)"""
    pos, erased, owner = [], [], []
    rows = []
    prev = []
    for r, s in enumerate(spec):
        (nx, ny, nz), d = GEN[s["gen"]]
        nrm = np.array([nx, ny, nz])
        u = np.cross(nrm, [0.3, 0.5, 0.8]); u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        share = s.get("share", 0)
        lms = list(prev[len(prev) - share:]) if share else []
        own = s["n"] - share
        for k in range(own):
            off = rng.uniform(-NOISE, NOISE)
            if k >= own - s.get("outliers", 0):
                off = rng.uniform(FAR, s.get("far", 3.0) * FAR) * (1 if k % 2 else -1)
            x = -d * nrm + rng.uniform(-2, 2) * u + rng.uniform(-2, 2) * v + off * nrm
            lms.append(len(pos))
            pos.append(x); erased.append(0); owner.append(r)
        mine = lms[share:]
        tail = len(mine) - s.get("outliers", 0)
        for lm in mine[tail - s.get("erased", 0):tail]:
            erased[lm] = 1
        for lm in mine[:s.get("unowned", 0)]:
            owner[lm] = -1
        for lm in mine[:s.get("foreign", 0)]:
            owner[lm] = r - 1
        if "nan_last" in s:
            s = dict(s, nan=nan_slot(np.array([pos[lm] for lm in lms]), seed + g, s["nan_last"], s.get("best_error", 1.0)))
        if s.get("nan") is not None:
            pos[lms[s["nan"]]] = np.array([np.nan, 0.0, 1.0])
        rows.append(dict(state=s["state"], eq=s.get("eq", (nx, ny, nz, d)), best_error=s.get("best_error", 1.0), lms=lms))
        prev = lms
    n_cap = max([len(r["lms"]) for r in rows] + [1])
    t = dict(pl_state=np.array([r["state"] for r in rows], np.uint8), pl_equation=np.array([r["eq"] for r in rows], np.float64).reshape(-1, 4),
             pl_best_error=np.array([r["best_error"] for r in rows], np.float64), pl_count=np.array([len(r["lms"]) for r in rows], np.int32),
             pl_lm=np.full((len(rows), n_cap), PAD, np.int32), pos_w=np.array(pos, np.float64).reshape(-1, 3), lm_erased=np.array(erased, np.uint8),
             lm_owner=np.array(owner, np.int32))
    for r, row in enumerate(rows):
        t["pl_lm"][r, :len(row["lms"])] = row["lms"]
    return t


def nan_slot(pos, seed, c, best_error):
    """a slot of a list of owned members whose NaN position makes update call c end with TOO_FEW_LEFT: the last hypothesis draws it (the plane
    ends with a NaN equation that keeps no member), an earlier one does not and is accepted"""
    n = len(pos)
    m = PR.sample_size(PR.UPDATE, n, PPR)
    drawn = [{PR.draw(seed, c, it, k, n) for k in range(m)} for it in range(ITERS)]
    for s in range(n):
        if s in drawn[-1] and any(s not in d for d in drawn[:-1]):
            q = pos.copy()
            q[s] = [np.nan, 0.0, 1.0]
            if PR.ransac(PR.UPDATE, q, np.full(n, PR.LM_OWNED, np.uint8), DIST, ERR, PPR, iters=ITERS, best_error_in=best_error, equation_in=[0, 0, 1, 0],
                         seed=seed, p=c)["status"] == PR.TOO_FEW_LEFT:
                return s
    raise AssertionError("no such slot: change the scene")


def pack(tables, NP_cap=None, n_cap=None, L=None):
    """the arrays of a call over these problems"""
    G = len(tables)
    NP = max([len(t["pl_state"]) for t in tables] + [NP_cap or 0])
    M = n_cap if n_cap is not None else 2 * max(t["pl_lm"].shape[1] for t in tables)           # room for the merges
    LL = max([len(t["lm_owner"]) for t in tables] + [L or 0])
    o = dict(pl_state=np.zeros((G, NP), np.uint8), pl_equation=np.zeros((G, NP, 4)), pl_best_error=np.ones((G, NP)), pl_count=np.zeros((G, NP), np.int32),
             pl_lm=np.full((G, NP, M), PAD, np.int32), pos_w=np.zeros((G, LL, 3)), lm_erased=np.ones((G, LL), np.uint8), lm_owner=np.full((G, LL), -1, np.int32))
    o["pl_equation"][:, :, 0] = 1.0
    for g, t in enumerate(tables):
        n, l, m = len(t["pl_state"]), len(t["lm_owner"]), min(t["pl_lm"].shape[1], M)
        for k in ("pl_state", "pl_equation", "pl_best_error", "pl_count"):
            o[k][g, :n] = t[k]
        o["pl_lm"][g, :n, :m] = t["pl_lm"][:, :m]
        for k in ("pos_w", "lm_erased", "lm_owner"):
            o[k][g, :l] = t[k]
    return o


def with_gaps(t, rows):
    """the problem t with its plane rows moved to `rows` (ascending) of a larger table; the gaps have IN_DB = 0 and a stale list"""
    NP = max(rows) + 1
    o = dict(t, pl_state=np.full(NP, VALID | NEED, np.uint8), pl_equation=np.tile(np.array([0.0, 0.0, 1.0, -1.0]), (NP, 1)), pl_best_error=np.ones(NP),
             pl_count=np.full(NP, 3, np.int32), pl_lm=np.zeros((NP, t["pl_lm"].shape[1]), np.int32))
    for k, r in enumerate(rows):
        for key in ("pl_state", "pl_equation", "pl_best_error", "pl_count", "pl_lm"):
            o[key][r] = t[key][k]
    o["lm_owner"] = np.array([rows[x] if x >= 0 else -1 for x in t["lm_owner"]], np.int32)
    return o


# the scenes of the census: name -> (plane specs, dict of per-problem settings)
SCENES = {
    # anchors: two lists of one generating plane become one row; two planes apart in offset and angle stay two
    "one_plane_two_lists": ([P(0, 60, outliers=2, far=1.25), P(0, 40, outliers=2, far=1.25)], {}),
    "two_planes_apart": ([P(0, 50), P(1, 45)], {}),
    # the two mixed outcomes: parallel and far, close and at an angle
    "mixed": ([P(0, 40), P(2, 40), P(3, 40)], {}),
    # equal sizes go to the candidate; the invalidated parent goes on and takes a third list
    "equal_sizes": ([P(0, 40), P(0, 40), P(0, 30)], {}),
    # one invalid row stepped over, the next invalid one tested (it lies on the parent's plane: an invalid candidate is merged)
    "skip_then_test": ([P(0, 50), P(1, 30, DEAD), P(0, 30, DEAD), P(1, 40)], {}),
    # runs of one, two and three invalid rows in the middle and an invalid row at the end
    "skip_runs": ([P(0, 50), P(4, 20, DEAD), P(1, 40), P(4, 20, DEAD), P(0, 30, DEAD), P(2, 40), P(4, 20, DEAD), P(0, 25, DEAD), P(4, 20, DEAD), P(3, 40),
                   P(4, 20, DEAD)], {}),
    # a landmark in two lists (planes at an angle that share members), moved by both
    "shared_members": ([P(0, 50), P(3, 50, share=12)], {}),
    # an entry already present at a merge, erased members, members without owner
    "already_present": ([P(0, 60, erased=4), P(0, 45, share=10, erased=3, unowned=5)], {}),
    # every arm of refine_planes: invalid, updated, update failed (too few points), small, kept; the erase clears owners another row holds
    "refine_arms": ([P(0, 50), P(1, 30, DEAD, foreign=30), P(2, 50, NEW), P(3, 10, NEW), P(4, 30), P(5, 40, NEW, unowned=40)], {}),
    # the update statuses that need their own thresholds or history
    "not_found": ([P(0, 50, NEW, best_error=0.0), P(1, 40)], {}),
    "error_above": ([P(0, 50, NEW), P(1, 40)], dict(error_thresh=1e-9)),
    "too_few_left": ([P(0, 40, NEW, nan_last=0), P(1, 40)], {}),
    "too_few_planes": ([P(0, 50, NEW)], {}),
}


def scene_tables(name, g=0, seed=SEED):
    spec, kw = SCENES[name]
    return build(spec, np.random.default_rng(sum(map(ord, name))), g, seed), kw


def census_call(names=None, seed=SEED):
    """(tables of one call over the scenes, dist_thresh (G,), error_thresh (G,), names)"""
    names = list(names or SCENES)
    ts, kws = zip(*[scene_tables(n, g, seed) for g, n in enumerate(names)])
    return pack(list(ts)), np.full(len(names), DIST), np.array([kw.get("error_thresh", ERR) for kw in kws]), names


def overflow_tables(over):
    """two lists of one plane whose merge holds exactly n_cap entries (over = 0) or one more (over = 1)"""
    t = build([P(0, 50), P(0, 30, share=4)], np.random.default_rng(77))
    return pack([t], n_cap=76 - over)


def run_ref(t, dist, err, stages=RR.STAGE_ALL, seed=SEED, iters=ITERS):
    G = t["pl_state"].shape[0]
    return [RR.run(t, g, float(np.broadcast_to(dist, (G,))[g]), float(np.broadcast_to(err, (G,))[g]), PPR, iters, DOT, FACTOR, seed, stages) for g in range(G)]


def call_kwargs(stages=RR.STAGE_ALL, seed=SEED, merge_cap=4, iters=ITERS):
    return dict(points_per_ransac=PPR, iters=iters, dot_product_threshold=DOT, offset_delta_factor=FACTOR, seed=seed, stages=stages, merge_cap=merge_cap)


def sentinel_out(t, merge_cap=4):
    G, NP = t["pl_state"].shape
    L = t["lm_owner"].shape[1]
    shape = dict(removed=(G, NP), merges=(G, merge_cap, 2), update_status=(G, NP), lm_changed=(G, L))
    return {k: np.full(shape.get(k, (G,)), RR.SENTINEL[k], RR.DTYPES[k]) for k in RR.SENTINEL}
